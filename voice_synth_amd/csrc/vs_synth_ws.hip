/*
 * vs_synth_ws.hip -- the wave-specialised fused kernels (the mapping and the arithmetic: vs_synth_one_wave.hip).
 * The same 64 utterances are served by SEVERAL wavefronts, each with
 * one job, coupled through the LDS ring and a few per-lane progress words.  This is what the fused
 * kind launches by default (vs_plan_create):
 *
 *   two roles (generator | filter) -- whatever does not suit the third role (no glottal noise; rings of
 *     barely one cycle: vs_plan_create_impl).  On grids that leave at least half of the chip's SIMDs empty
 *     every wavefront has a SIMD of its own and a launch takes max(generator, filter) instead of their sum;
 *
 *   three roles (open phase | noise | filter) -- full grids over deep rings (BASELINE config 3: 1024
 *     groups on 1024 SIMDs): four groups per 768-thread workgroup, one workgroup per CU, wavefronts laid out
 *     role-major so that every SIMD hosts the three wavefronts of ONE group (a workgroup's wavefronts
 *     are dealt to the CU's four SIMDs cyclically: w, w+4, w+8 share a SIMD).  Why three: a lone
 *     wavefront issues one instruction -- vector, scalar or LDS alike -- every ~5.25 cycles, and the
 *     filter wavefront at raised priority leaves a second wavefront about a quarter of that
 *     (tools/ubench/ubench3.hip), so a launch of the two-role kernel takes about 0.74 x filter + generator:
 *     whatever the generator cannot do in the filter's shadow it does ALONE on its SIMD while the
 *     filter sleeps.  Two generator wavefronts side by side run at 5.25 and 11 cycles per
 *     instruction (ubench4.hip), i.e. that part goes ~1.5x faster when the generator's work is cut
 *     in two: jitter / shimmer / both flanks here, the closed phase's noise there.
 *     Half-filled chips with glottal noise (BASELINE config 4 sharded over 8 GPUs: 512 groups on 1024 SIMDs; the
 *     16384-utterance chunks of the pipelines) take three roles too, laid out so that the filter wavefront -- the
 *     bound in exact arithmetic -- has a SIMD to itself and the two generator wavefronts share the next one
 *     (VS_WS_LAYOUT_SPREAD_2X3, vs_device.h: TWO groups per workgroup, the launcher refuses anything else; a grid of
 *     at most one group per CU runs role-major with one group per workgroup, a SIMD per wavefront), over rings of 2.4 cycles.
 *
 * Hand-off (workgroup scope, LDS only), per lane l:
 *   gpub[l] = samples of l that are complete in the ring     (written by the generator / by the noise wavefront)
 *   npub[l] = samples of l the filter has read from the ring  (written by the filter wavefront)
 *   three roles: oseq[l] / otak[l] = orders posted by the open-phase wavefront / taken by the noise
 *   wavefront, ord[0..2][l] = the order (vs_post_order): which draws, which samples, what width.
 * The LDS executes one wavefront's operations in order, so "ring writes, then gpub" on one side and
 * "gpub read, then ring reads" on the other is a release/acquire pair; the fences keep the compiler
 * from reordering.  A cycle's slots [g, g+T) are written only when g - npub + T <= C (T = the cycle's
 * period, fixed by vs_cycle_scalars), i.e. never over samples the filter has not consumed.  In the
 * three-role kernel two wavefronts write the ring at the same time -- cycle c's noise and cycle
 * c+1's flanks -- so the noise wavefront stops exactly at the end of its cycle (vs_noise_trips<TAIL>),
 * while the open-phase wavefront only ever runs past a phase INSIDE its own cycle and finishes all
 * of that before it posts the order.
 *
 * Progress: a lane that is short of 24 samples always has room for its next cycle, and a generator
 * round starts whenever such a lane exists; if no lane has room every lane holds more than 24 samples
 * and the filter runs.  Spins are bounded (args.spin_limit polls, then the error word of the launch
 * is set and the wavefront leaves) so that a protocol bug cannot hang the device.
 */
#include "vs_kernel_table.h"
#include "vs_dev_generator.h"
#include "vs_dev_filter.h"

/* s_sleep units of 64 cycles between two polls of a waiting wavefront.  A polling wavefront takes issue slots from the
 * working ones, a sleeping one reacts late.  Two roles on a full grid (BASELINE config 5): 32 (A/B 1, 2, 8, 32: best by
 * ~2 %; 8 is 1.2 % slower).  Three roles: 8 -- each wavefront has half the work per sample, hand-offs are twice as
 * frequent, and a late reaction costs more than the polls (config 3: 2.81-2.86 against 2.88-2.91 ms at 32, four and
 * five same-box repetitions; 4 .. 16 are alike; profiles/r04_poll_sleep_ab.txt).  Half-filled chips do not care.
 * -DVS_POLL_SLEEP=n sets both (A/B builds). */
#ifdef VS_POLL_SLEEP
#define VS_POLL_SLEEP_2 VS_POLL_SLEEP
#define VS_POLL_SLEEP_3 VS_POLL_SLEEP
#else
#define VS_POLL_SLEEP_2 32
#define VS_POLL_SLEEP_3 8
#endif
/* (s_sleep takes an immediate: one call site per value) */
template <bool THREE>
__device__ __forceinline__ void vs_poll_sleep()
{
  if (THREE) __builtin_amdgcn_s_sleep(VS_POLL_SLEEP_3);
  else __builtin_amdgcn_s_sleep(VS_POLL_SLEEP_2);
}

/* what every role of a group needs to find its lane, its ring and its progress words */
struct VsGroup {
  const VsDevLane *L;
  int16_t *ring;
  double *ltab;
  int *gpub, *npub;
  VsOrderBox ord;
  long group, row;
  int lane, N, C;
  int ltab_entries; /* doubles reserved for this group's cos rows (the launch's, or the group's own over mixed rings) */
  bool valid;
};

/* The generator role of the two-role kernel (SPLIT = false: whole cycles) and the open-phase role of
 * the three-role kernel (SPLIT = true: jitter, shimmer and both flanks; the cycle's noise leaves as
 * an order, and progress is published by the noise wavefront only). */
template <bool SPLIT>
__device__ __forceinline__ void vs_generator_wave(const VsKernelArgs &args, const VsGroup &g)
{
  const int lane = g.lane, N = g.N, C = g.C;
  VsCfg c;
  VsGen s;
  VsDiag dg;
#ifdef VS_DIAG
#pragma unroll
  for (int k = 0; k < 8; ++k) dg.acc[k] = 0;
  dg.rounds = dg.attend = 0;
  dg.t = vs_stamp();
#endif
  vs_load_cfg(g.L, c, s);
  const bool uni = vs_stage_cos_rows<true>(g.L, c, g.ltab, args.costab, g.ltab_entries, lane, g.valid, args);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); /* own staging writes before own row reads */
  VsRoundKeys rk; /* two roles: this wavefront draws the noise itself (three: the noise wavefront has its own) */
  if (!SPLIT) vs_round_keys(c.key0, c.key1, rk);
  int spins = 0;
  /* A poll that cannot end differently from the last one is cut short: whether a round starts depends
   * on this wavefront's own state (which only a round changes) and on two words per lane written by
   * the others -- npub and, three roles, otak.  While neither has moved the wavefront goes back to
   * sleep after two LDS reads and a compare instead of the ~30 instructions of the full evaluation;
   * an idle open-phase wavefront polls ~2000 times per launch, and every instruction it issues is
   * taken from the two that work (profiles/r03_kernel_experiments.txt). */
  int prev_seen = -1, prev_taken = -1;
  bool dirty = true; /* own state changed since the last full evaluation */
  /* tests (vs_tuning.fault): a generator that never publishes -- the bounded waits of the other
   * wavefronts must run out and reach the caller as VS_ERR_INTERNAL */
  const bool withhold = args.fault == VS_FAULT_WITHHOLD_PROGRESS;
  while (!withhold) {
#ifdef VS_TIMING_GENERATOR_ONLY
    const int n_seen = s.g; /* timing build: the generator alone, never short of room */
#else
    const int n_seen = __hip_atomic_load(&g.npub[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
    int taken = 0;
    if (SPLIT) taken = __hip_atomic_load(&g.ord.otak[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (!dirty && !__any((n_seen != prev_seen) || (taken != prev_taken))) {
      vs_poll_sleep<SPLIT>();
      VS_DIAG_ADD(dg, 6)
      if (++spins > args.spin_limit) {
        if (args.err && lane == 0) atomicOr(args.err, 1);
        break;
      }
      continue;
    }
    prev_seen = n_seen;
    prev_taken = taken;
    dirty = false;
    const bool need = g.valid && (s.g < N);
    if (!__any(need)) break;
    if (need && !s.pend) vs_cycle_scalars(c, s, dg); /* fixes the next period s.T */
    bool want = need && (s.g - n_seen + s.T + VS_TRASH_ROWS <= C);
    /* ... and, three roles, one of the lane's order boxes is free */
    if (SPLIT) want = want && (s.posted - taken < VS_ORDER_DEPTH);
    const bool hungry = want && (s.g - n_seen < args.gen_low); /* its filter would run dry during a round */
    const int n_need = __builtin_popcountll(__ballot(need));
    const int n_want = __builtin_popcountll(__ballot(want));
    if ((n_want > 0) && ((n_want * 64 >= n_need * args.gen_min) || __any(hungry))) {
#ifdef VS_DIAG
      dg.rounds += 1;
      dg.attend += (unsigned long long)n_want;
#endif
      if (SPLIT) {
        if (want) vs_cycle_emit<false, false, true>(c, s, g.ring, C, lane, N, g.ltab, uni, args.costab, nullptr, 0, dg, nullptr, g.ord);
      } else {
        if (want) vs_cycle_emit<false, true, false>(c, s, g.ring, C, lane, N, g.ltab, uni, args.costab, nullptr, 0, dg, &g.gpub[lane], VsOrderBox(), &rk);
        VS_LDS_RELEASE();
        __hip_atomic_store(&g.gpub[lane], s.g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      spins = 0;
      dirty = true;
    } else {
      vs_poll_sleep<SPLIT>();
      VS_DIAG_ADD(dg, 6)
      if (++spins > args.spin_limit) {
        if (args.err && lane == 0) atomicOr(args.err, 1);
        break;
      }
    }
  }
#ifdef VS_DIAG
  if (args.diag && lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) args.diag[(size_t)g.group * 16 + k] = dg.acc[k];
    args.diag[(size_t)g.group * 16 + 9] = dg.rounds; /* slots 9, 10: unused by the filter wavefront */
    args.diag[(size_t)g.group * 16 + 10] = dg.attend;
  }
#endif
  if (args.ncyc && g.valid) args.ncyc[g.row] = s.cyc;
}

/* The noise role of the three-role kernel: takes the orders of the open-phase wavefront, adds the
 * closed phase's noise (flowgen_shimmer.c:385-406, vs_noise_trips) and is the one that publishes a
 * lane's progress to the filter: the open phase when it takes the order, the closed phase trip by
 * trip.  The round keys of a lane's Philox stream are made once per launch here. */
__device__ __forceinline__ void vs_noise_wave(const VsKernelArgs &args, const VsGroup &g)
{
  const int lane = g.lane, N = g.N, C = g.C;
  VsRoundKeys rk;
  vs_round_keys(g.L->key0, g.L->key1, rk);
  const int dcs = g.L->dcs;
  int taken = 0; /* orders of this lane dealt with */
  int gend = 0;  /* samples of this lane that are complete = where its next cycle starts */
  int wpos = 0;  /* ring slot of sample gend */
  int spins = 0;
#ifdef VS_DIAG
  VsDiag dg;
#pragma unroll
  for (int k = 0; k < 8; ++k) dg.acc[k] = 0;
  dg.rounds = dg.attend = 0;
  dg.t = vs_stamp();
#endif
  for (;;) {
    const bool open = g.valid && (gend < N);
    if (!__any(open)) break;
    const int posted = __hip_atomic_load(&g.ord.oseq[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const bool have = open && (posted != taken);
    if (__any(have)) {
      if (have) {
        const int *box = g.ord.w + (taken & (VS_ORDER_DEPTH - 1)) * (3 * VS_WAVE) + lane;
        const uint32_t d0 = (uint32_t)box[0];
        const int w1 = box[VS_WAVE];
        const int NDW = box[2 * VS_WAVE];
        taken += 1;
        /* the three reads above precede this store in the LDS queue: the box is free again */
        VS_LDS_RELEASE();
        __hip_atomic_store(&g.ord.otak[lane], taken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int T3 = w1 & 0xFFFF, T = (int)((unsigned)w1 >> 16);
        const int m = T - T3;
        /* the open phase [0, T3) of this cycle is in the ring (it was before the order was posted) */
        __hip_atomic_store(&g.gpub[lane], gend + T3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__any(m > 0)) {
          vs_noise_trips<true, true>(g.ring, C, lane, rk, vs_noise_consts(NDW, dcs), d0, m, wpos, T3, gend,
                                     &g.gpub[lane]);
        }
        gend += T;
        wpos += T; /* T <= ring_slots */
        if (wpos >= C) wpos -= C;
      }
      spins = 0;
      VS_DIAG_ADD(dg, 4)
    } else {
      vs_poll_sleep<true>();
      VS_DIAG_ADD(dg, 6)
      if (++spins > args.spin_limit) {
        if (args.err && lane == 0) atomicOr(args.err, 4);
        break;
      }
    }
  }
#ifdef VS_DIAG
  if (args.diag && lane == 0) { /* slots 11, 12: unused by the filter wavefront */
    args.diag[(size_t)g.group * 16 + 11] = dg.acc[4];
    args.diag[(size_t)g.group * 16 + 12] = dg.acc[6];
  }
#endif
}

/* The filter role: super-steps of 24 samples for every lane that holds them (vs_superstep).
 * PARTIAL: groups whose threshold is below 64 lanes run super-steps with the ready lanes only (the
 * two-role kernel); without it every group waits for all of its live lanes (the three-role kernel:
 * the second copy of the window that a partial super-step needs does not fit its 168 registers). */
template <int ARITH, bool PRE1, bool PARTIAL, bool POW>
__device__ __forceinline__ void vs_filter_wave(const VsKernelArgs &args, const VsGroup &g)
{
  const int lane = g.lane, N = g.N, C = g.C;
  const VsDevLane *__restrict__ L = g.L;
  int16_t *ring = g.ring;
  int *gpub = g.gpub, *npub = g.npub;
  const bool valid = g.valid;
  /* When wavefronts share a SIMD (full grids), VALU issue goes to the higher priority first: the
   * filter is the longest of the instruction streams, so it issues as if it were alone and the
   * others fill the slots it leaves.  Without this the hardware prefers the OLDEST wavefront -- the
   * generator -- and the launch takes longer (profiles/r02_ws_full_grid_sweep.txt). */
  if (args.ws_filter_prio >= 3) __builtin_amdgcn_s_setprio(3);
  else if (args.ws_filter_prio == 2) __builtin_amdgcn_s_setprio(2);
  else if (args.ws_filter_prio == 1) __builtin_amdgcn_s_setprio(1);
  /* VS_ARITH_F32: the window and the taps are the packed single-precision ones (VsF32Filter, vs_dev_filter.h); the double
   * ones below are never touched and compile away */
  constexpr bool F32 = (ARITH == VS_ARITH_F32);
  constexpr int DARITH = F32 ? VS_ARITH_FMA : ARITH;
  VsF32Filter f32;
  double a[VS_ORDER + 1];
  if (F32) vs_f32_load(args.taps, L, f32);
  else vs_load_taps<DARITH>(args.taps, L, a);
  const double gain = L->gain;
  const double pre = L->pre;
  int16_t *orow = args.out + g.row * args.out_pitch;
  const int ready_min = (args.ready_min > 0) ? args.ready_min : __builtin_amdgcn_readfirstlane(L->ready_min);
#ifdef VS_DIAG
  VsDiag dg;
#pragma unroll
  for (int k = 0; k < 8; ++k) dg.acc[k] = 0;
  dg.t = vs_stamp();
#endif
  if (!PARTIAL || ready_min >= VS_WAVE) {
    /* Every live lane must be ready (the threshold of deep rings, BASELINE config 3): all lanes
     * of the group then share one position n, the loop is wave-uniform, and the super-step runs
     * under the FULL exec mask -- lanes beyond n_lanes filter whatever their ring column holds
     * and only their stores are masked.  What that buys: the window y[] is updated in place.
     * Under a divergent "if (ready)" the compiler has to keep the old window alive for the
     * lanes that sit out and copies all 24 doubles in and out of every super-step (2 of 55
     * vector instructions per sample). */
    double y[VS_SS];
#pragma unroll
    for (int j = 0; j < VS_SS; ++j) y[j] = 0.0; /* vowel_new.c:222-224 */
    /* A wait that runs out (a protocol bug, or the fault injected by the tests) sets the error word
     * and stops waiting: the remaining super-steps run on whatever the ring holds, the launch ends
     * and vs_plan_status() reports it.  No second way out of the loop -- a "break" here would make
     * the old and the new window meet at the loop latch, and the compiler would copy it again. */
    bool gave_up = false;
    int rslot = 0;
    /* waits until every live lane holds the 24 samples from n on */
    auto await = [&](int n) {
      for (int polls = 0; !gave_up; ++polls) {
#ifdef VS_TIMING_FILTER_ONLY
        const int g_seen = N; /* timing build: the filter alone, never short of input */
#else
        const int g_seen = __hip_atomic_load(&gpub[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
        const bool ready = !valid || (g_seen - n >= VS_SS) || (g_seen >= N);
        if (__all(ready)) break;
        vs_poll_sleep<!PARTIAL>();
        VS_DIAG_ADD(dg, 6)
        if (polls > args.spin_limit) {
          if (args.err && lane == 0) atomicOr(args.err, 2);
          gave_up = true;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    /* the ring reads of the super-step precede this store in the LDS queue: the slots are free */
    auto release = [&](int n_done) {
      rslot += VS_SS;
      if (rslot >= C) rslot = 0;
      VS_LDS_RELEASE();
      __hip_atomic_store(&npub[lane], n_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    /* Lanes beyond n_lanes store to a row of their own that nobody reads, and the super-steps that
     * store sample by sample (the last one of a length that is no multiple of 24; all of them when rows
     * are not 4-byte aligned) run in a loop of their own: no branch is left inside a super-step, and
     * without one the compiler keeps each ring read together with its sign extension (DS_READ_I16
     * instead of DS_READ_U16 + V_BFE_I32: 16 instructions per super-step) and drops the exec masks
     * around the 16-byte stores. */
    if (!valid) orow = args.sink;
    const int n_whole = (args.vec_ok != 0) ? (N / VS_SS) * VS_SS : 0;
    /* POW: vowel -n's frame powers on the way (VsFramePower, vs_dev_filter.h) -- every lane of the launch has frames of
     * args.pow_lframe samples, and the lanes of this wavefront share one position, so where a frame ends is a scalar */
    VsFramePower fp;
    int f_len = 0, f_left = 0; /* length of the frame the next super-step starts in; what is left of it */
    if (POW) {
      fp.sum = fp.done = 0.0f;
      fp.frame = 0;
      fp.bad = fp.requirk = false;
      fp.lanes = args.lanes;
      fp.ondw = args.ondw;
      fp.ondw_pitch = args.ondw_pitch;
      fp.first_lane = g.group * VS_WAVE;
      fp.n_lanes = args.n_lanes;
      f_len = f_left = (args.pow_lframe < N) ? args.pow_lframe : N;
    }
    int n = 0;
    for (; n < n_whole; n += VS_SS) {
      VS_DIAG_ADD(dg, 7)
      await(n);
      int outv[VS_SS];
      vs_u32x4 xpre[VS_SS / 8]; /* only the filter-only kind prefetches */
      if (POW) {
        fp.tb = (f_left <= VS_SS) ? f_left : 0;
        fp.len = f_len;
        fp.force = (args.fault == VS_FAULT_REROUND) && ((n / VS_SS) % 7 == 3);
      }
      if constexpr (F32)
        vs_superstep_f32<PRE1, 1, POW>(f32, ring + rslot * VS_WAVE + lane, orow, n, N, true, &fp);
      else
        vs_superstep<DARITH, VS_KIND_SYNTH, PRE1, true, 1, PARTIAL, POW>(a, y, gain, pre, ring + rslot * VS_WAVE + lane, nullptr, orow, n,
                                                                         N, true, outv, xpre, true, &fp);
      if (POW) {
        if (fp.tb) { /* a frame ended behind sample tb - 1; the rest of the super-step went to the next one's sum */
          vs_frame_power_store(fp, fp.bad || fp.requirk);
          fp.frame += 1;
          fp.bad = fp.requirk;
          const int rest = N - (n + fp.tb);
          f_len = (args.pow_lframe < rest) ? args.pow_lframe : rest;
          f_left = f_len - (VS_SS - fp.tb);
        } else {
          fp.bad = fp.bad || fp.requirk;
          f_left -= VS_SS;
        }
        fp.requirk = false;
      }
      release(n + VS_SS);
      VS_DIAG_ADD(dg, 0)
    }
    /* frames [0, fp.frame) have their width (or NaN) in the table; the one in progress and whatever the sample-by-sample
     * super-steps below complete are the streaming pass's */
    if (POW && valid) args.odone[g.row] = fp.frame;
    for (; n < N; n += VS_SS) {
      VS_DIAG_ADD(dg, 7)
      await(n);
      int outv[VS_SS];
      vs_u32x4 xpre[VS_SS / 8];
      if constexpr (F32)
        vs_superstep_f32<PRE1, 0, false>(f32, ring + rslot * VS_WAVE + lane, orow, n, N, true);
      else
        vs_superstep<DARITH, VS_KIND_SYNTH, PRE1, true, 0>(a, y, gain, pre, ring + rslot * VS_WAVE + lane, nullptr, orow, n,
                                                           N, false, outv, xpre, true);
      release(n + VS_SS);
      VS_DIAG_ADD(dg, 0)
    }
  } else {
    /* shallower rings: a super-step as soon as ready_min/64 of the live lanes hold 24 samples; every
     * lane has its own position n (no frame powers on the way: all of them are the streaming pass's) */
    if (POW && valid) args.odone[g.row] = 0;
    double y[VS_SS];
#pragma unroll
    for (int j = 0; j < VS_SS; ++j) y[j] = 0.0; /* vowel_new.c:222-224 */
    int n = 0, rslot = 0, spins = 0;
    bool live = valid;
    while (__any(live)) {
      VS_DIAG_ADD(dg, 7)
#ifdef VS_TIMING_FILTER_ONLY
      const int g_seen = N;
#else
      const int g_seen = __hip_atomic_load(&gpub[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const bool ready = live && ((g_seen - n >= VS_SS) || (g_seen >= N));
      const int n_live = __builtin_popcountll(__ballot(live));
      const int n_ready = __builtin_popcountll(__ballot(ready));
      if ((n_ready > 0) && (n_ready * 64 >= n_live * ready_min)) {
        /* Every lane has its own n, so "all 24 samples lie inside the row" is a per-lane question -- but
         * one that only a lane's LAST super-step answers with no (N is no multiple of 24), or every one
         * when rows are not 4-byte aligned.  Asked once per super-step for the whole wavefront it leaves
         * the common case without the 24 per-sample bounds tests and the exec masks around them. */
        const bool inside = (args.vec_ok != 0) && (n + VS_SS <= N);
        if (__all(!ready || inside)) {
          if (ready) {
            int outv[VS_SS];
            vs_u32x4 xpre[VS_SS / 8]; /* only the filter-only kind prefetches */
            if constexpr (F32)
              vs_superstep_f32<PRE1, 1, false>(f32, ring + rslot * VS_WAVE + lane, orow, n, N, true);
            else
              vs_superstep<DARITH, VS_KIND_SYNTH, PRE1, true, 1, PARTIAL>(a, y, gain, pre, ring + rslot * VS_WAVE + lane, nullptr, orow,
                                                                          n, N, true, outv, xpre);
          }
        } else {
          if (ready) {
            int outv[VS_SS];
            vs_u32x4 xpre[VS_SS / 8];
            if constexpr (F32)
              vs_superstep_f32<PRE1, 0, false>(f32, ring + rslot * VS_WAVE + lane, orow, n, N, true);
            else
              vs_superstep<DARITH, VS_KIND_SYNTH, PRE1, true>(a, y, gain, pre, ring + rslot * VS_WAVE + lane, nullptr, orow,
                                                              n, N, args.vec_ok != 0, outv, xpre);
          }
        }
        if (ready) {
          rslot += VS_SS;
          if (rslot >= C) rslot = 0;
          n += VS_SS;
          if (n >= N) live = false;
        }
        /* the ring reads above precede this store in the LDS queue: the slots are free */
        VS_LDS_RELEASE();
        __hip_atomic_store(&npub[lane], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        spins = 0;
        VS_DIAG_ADD(dg, 0)
      } else {
        vs_poll_sleep<!PARTIAL>();
        VS_DIAG_ADD(dg, 6)
        if (++spins > args.spin_limit) {
          if (args.err && lane == 0) atomicOr(args.err, 2);
          break;
        }
      }
    }
  }
#ifdef VS_DIAG
  if (args.diag && lane == 0) {
    args.diag[(size_t)g.group * 16 + 8] = dg.acc[0];
    args.diag[(size_t)g.group * 16 + 14] = dg.acc[6];
    args.diag[(size_t)g.group * 16 + 15] = dg.acc[7];
  }
#endif
}

/* ROLES wavefronts per group of 64 utterances, args.ws_pairs groups per workgroup, wavefronts laid
 * out role-major: role = wavefront / groups.  Two roles: 0 generator, 1 filter.  Three roles: 0 open
 * phase, 1 noise, 2 filter (the hardware prefers the older of two wavefronts of equal priority:
 * open phase before noise is the better order, tools/ubench/ubench4.hip). */
template <int ARITH, bool PRE1, int ROLES, bool POW>
__device__ __forceinline__ void vs_synth_ws_body(const VsKernelArgs &args)
{
  extern __shared__ __attribute__((aligned(16))) int16_t lds_base[];

  const int widx = (int)threadIdx.x >> 6;
  int ngroups, role, slot;
  if (ROLES == 3 && args.ws_layout == VS_WS_LAYOUT_SPREAD_2X3) {
    /* eight wavefronts: F0 O0 F1 O1 -- N0 -- N1 (vs_device.h); role -1 = nothing to do */
    const int simd = widx & 3, second = widx >> 2;
    ngroups = 2;
    slot = simd >> 1;
    role = (simd & 1) ? (second ? 1 : 0) : (second ? -1 : 2);
  } else {
    ngroups = (int)blockDim.x / (ROLES * VS_WAVE);
    role = widx / ngroups;
    slot = widx - role * ngroups;
  }
  VsGroup g;
  g.lane = (int)threadIdx.x & (VS_WAVE - 1);
  g.group = (long)blockIdx.x * (long)ngroups + slot;
  g.C = args.ring_slots;
  g.ltab_entries = args.ltab_entries;
  g.ring = lds_base + (size_t)slot * (size_t)(args.ws_pair_bytes / sizeof(int16_t));
  if (args.group_map) {
    /* mixed rings (vs_device.h, VsGroupSlot): this slot's group, ring depth and LDS region come from the plan's
     * table -- one scalar load, everything stays wave-uniform */
    const VsGroupSlot gs = args.group_map[(size_t)blockIdx.x * (size_t)ngroups + (size_t)slot];
    g.group = (gs.group >= 0) ? (long)gs.group : (((long)args.n_lanes + VS_WAVE - 1) / VS_WAVE); /* none: beyond the batch */
    g.C = __builtin_amdgcn_readfirstlane(gs.ring_slots);
    g.ring = lds_base + (size_t)__builtin_amdgcn_readfirstlane(gs.lds_off) / sizeof(int16_t);
    g.ltab_entries = __builtin_amdgcn_readfirstlane(gs.ltab_entries);
  }
  const long gl = g.group * VS_WAVE + g.lane;
  g.valid = gl < (long)args.n_lanes;
  g.L = args.lanes + (g.valid ? gl : (long)args.n_lanes - 1);
  g.N = args.n_samples;
  g.ltab = (double *)(g.ring + (size_t)(g.C + VS_TRASH_ROWS) * VS_WAVE);
  g.gpub = (int *)(g.ltab + g.ltab_entries);
  g.npub = g.gpub + VS_WAVE;
  g.ord.oseq = g.npub + VS_WAVE;
  g.ord.otak = g.ord.oseq + VS_WAVE;
  g.ord.w = g.ord.otak + VS_WAVE;
  g.row = (long)g.L->row;

  if (role == 0) {
    g.gpub[g.lane] = 0;
    g.npub[g.lane] = 0;
    if (ROLES == 3) {
      g.ord.oseq[g.lane] = 0;
      g.ord.otak[g.lane] = 0;
    }
  }
  __syncthreads();
  if (role < 0) return; /* the two spare wavefronts of the spread layout */
  /* a slot without a group (the last workgroup of a grid that is no multiple of its groups; an empty slot of the
   * mixed-rings table): nothing to synthesise -- its filter wavefront used to run all N samples into the sink row */
  if (g.group * VS_WAVE >= (long)args.n_lanes) return;

#ifdef VS_TIMING_GENERATOR_ONLY
  if (role == ROLES - 1) return;
#endif
#ifdef VS_TIMING_FILTER_ONLY
  if (role != ROLES - 1) return;
#endif
  if (role == ROLES - 1) vs_filter_wave<ARITH, PRE1, ROLES == 2, POW>(args, g);
  else if (ROLES == 3 && role == 1) vs_noise_wave(args, g);
  else vs_generator_wave<ROLES == 3>(args, g);
}
template <int ARITH, bool PRE1, int ROLES>
__global__ void __launch_bounds__(ROLES * 4 * VS_WAVE) vs_synth_ws_kernel(VsKernelArgs args)
{
  vs_synth_ws_body<ARITH, PRE1, ROLES, false>(args);
}
/* the same with vowel -n's frame powers taken along by the filter wavefronts (VsFramePower, vs_dev_filter.h) */
template <int ARITH, bool PRE1, int ROLES>
__global__ void __launch_bounds__(ROLES * 4 * VS_WAVE) vs_synth_ws_pow_kernel(VsKernelArgs args)
{
  vs_synth_ws_body<ARITH, PRE1, ROLES, true>(args);
}

#define VS_E_WS(A, P, R) {VS_KERNEL_ID(VS_KF_WS, A, P, R, 0), vs_synth_ws_kernel<A, P, R>}
#define VS_E_WS_POW(A, P, R) {VS_KERNEL_ID(VS_KF_WS_POW, A, P, R, 0), vs_synth_ws_pow_kernel<A, P, R>}
/* <ARITH, PRE1, ROLES>, with and without the frame powers of vowel -n */
#define VS_E_WS_ALL(A)                                                                                         \
  VS_E_WS(A, false, 2), VS_E_WS(A, true, 2), VS_E_WS(A, false, 3), VS_E_WS(A, true, 3), VS_E_WS_POW(A, false, 2), \
      VS_E_WS_POW(A, true, 2), VS_E_WS_POW(A, false, 3), VS_E_WS_POW(A, true, 3)
const VsKernelEntry vs_kernel_table_ws[] = {VS_E_WS_ALL(VS_ARITH_EXACT), VS_E_WS_ALL(VS_ARITH_FMA), VS_E_WS_ALL(VS_ARITH_F32), {0, nullptr}};
