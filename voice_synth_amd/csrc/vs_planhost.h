/*
 * vs_planhost.h -- the device-free half of plan creation and of a plan's launches (csrc/vs_planhost.c), shared with
 * vs_api.c and the launchers of vs_kernels.hip.
 */
#ifndef VS_PLANHOST_H
#define VS_PLANHOST_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_device.h"

#ifdef __cplusplus
extern "C" {
#endif
/* A[0..40] of the lane's filter: the table or the explicit set, zeros behind its order */
int vs_lane_taps(const vs_lane *lane, double *A);
/* the ten tables by number (csrc/vs_host.c): 0..9, -1 / 0 for anything else */
int vs_vowel_index(int vowel);
int vs_vowel_by_index(int index);
/* The plan's tap table: rows 0..9 the ten tables, then one row per record whose tap_row is -1 (a coefficient set of the
 * lane's own, taken from lanes[record.row]; the record learns its row).  *taps is malloc'ed ([*rows][22] doubles, A[1..22]),
 * the caller frees it. */
int vs_tap_table_build(const vs_lane *lanes, VsDevLane *dl, size_t n_lanes, size_t n_custom, double **taps, size_t *rows);
bool vs_lane_is_wide(const vs_lane *lane);
/* VsDevLane.lframe_magic: the multiplier behind "sample index / frame length" in vs_out_noise_kernel */
uint32_t vs_lframe_magic(int Lframe);
/* one lane -> the record the kernels read (validated); the filter-only form fills what vowel reads */
int vs_expand_lane(const vs_lane *lane, int32_t row, VsDevLane *d);
int vs_expand_filter_lane(const vs_lane *lane, int32_t row, VsDevLane *d);
/* what a plan needs to know about its batch as a whole: gathered by the threads that make the records, so that the
 * plan does not walk all of them again for every question */
typedef struct VsBatchStats {
  int max_T2;       /* longest cos row */
  int tmax;         /* longest period any lane's rejection test admits (VsDevLane.tbound) */
  int min_lframe;   /* shortest frame (> 0) of the batch, 0: none */
  int max_lframe;   /* longest frame; == min_lframe (and no_lframe 0): every lane has the same */
  int no_lframe;    /* some lane has no frame at all (fs < 2000) */
  int any_onoise;   /* some lane asks for vowel -n */
  int pre1;         /* every lane has pre_emphasis == 1.0 */
  int wide;         /* some lane carries a coefficient set of 23..40 taps */
  size_t n_noisy;   /* lanes with glottal noise (VS_DF_NOISE) */
  size_t n_custom;  /* lanes that bring a coefficient set of their own (tap_row -1) */
} VsBatchStats;
/* all lanes, cut over up to 16 host threads for batches >= 8192; the failure of the lowest lane wins; stats may be NULL */
int vs_expand_all(const vs_lane *lanes, VsDevLane *dl, size_t n_lanes, int filter_only);
int vs_expand_all_stats(const vs_lane *lanes, VsDevLane *dl, size_t n_lanes, int filter_only, VsBatchStats *stats);
/* the source records in the order the kernels want -- stable by (P, T2, jitter / shimmer / noise on) -- written
 * straight into place: *order (malloc'ed, caller frees; NULL = input order: a homogeneous batch) says which lane
 * record i comes from (vs_kernel_order), vs_expand_all_ordered does both */
int vs_kernel_order(const vs_lane *lanes, size_t n_lanes, uint32_t **order);
int vs_expand_all_ordered(const vs_lane *lanes, VsDevLane *dl, size_t n_lanes, int *reordered, VsBatchStats *stats);
/* What plan creation keeps between calls (one per context): up to 16 worker threads that sleep between plans, the
 * record buffers, keys and sort arrays.  vs_expand_all_ordered_ws makes the records of a batch in it -- source kinds in
 * kernel order, filter-only in input order -- and *dl points into the workspace until the next call. */
typedef struct VsPlanWs VsPlanWs;
VsPlanWs *vs_planws_create(void);
void vs_planws_destroy(VsPlanWs *ws);
/* where the record buffers of big batches (8192 lanes and more) come from -- the context hands in page-locked memory, so
 * that their upload is a DMA transfer that runs next to a kernel; before the first batch only, NULL = malloc */
typedef void *(*vs_planws_alloc_fn)(void *user, size_t bytes);
typedef void (*vs_planws_free_fn)(void *user, void *ptr);
void vs_planws_set_big_allocator(VsPlanWs *ws, vs_planws_alloc_fn alloc, vs_planws_free_fn release, void *user);
int vs_expand_all_ordered_ws(VsPlanWs *ws, const vs_lane *lanes, size_t n_lanes, int filter_only, VsDevLane **dl,
                             int *reordered, VsBatchStats *stats);
void vs_cos_row(int T2, double *row);
/* ring capacity (slots per utterance) and super-step threshold for periods up to tmax */
int vs_ring_policy_for(int group_lanes, int tmax, int cap, int *slots, int *ready_min, int request, double depth);
int vs_ring_policy(int tmax, int cap, int *slots, int *ready_min);
int vs_ring_slots_for(int tmax, int *slots);
/* Mixed rings (vs_device.h, VsGroupSlot): the table of a full grid whose 64-utterance groups (lanes [64 g, 64 g + 64) of
 * the sorted records) differ in period -- every group with the ring depth ITS periods need (1.7 cycles, at least
 * floor_slots) and its own cos-row reservation, the groups dealt to workgroups of four in snake order of their longest
 * period.  VS_OK: *gmap (malloc'ed, [*n_wg][4], caller frees) with every group exactly once, the rest -1; *max_lds = the
 * largest workgroup's LDS bytes (<= VS_LDS_LIMIT), *c_min / *c_max the shallowest / deepest ring.  VS_ERR_UNSUPPORTED:
 * some workgroup would not fit (nothing allocated).  VS_ERR_NOMEM. */
int vs_mixed_rings_build(const VsDevLane *dl, size_t n_lanes, int floor_slots, VsGroupSlot **gmap, size_t *n_wg,
                         size_t *max_lds, int *c_min, int *c_max);

/* The tables of a synthesis plan, from its records in their final order: one cos row per distinct T2 in the order the
 * records meet them (none for a filter-only plan; VsDevLane.tab_off is written), a spare entry, the tap table from
 * taps_off on (VsDevLane.tap_row is written for the lanes' own sets) -- costab_len doubles in all, what goes to the
 * device --, ltab_entries = the cos rows the worst wavefront stages, and for a batch with wide sets the 40 taps of every
 * record (awide, else NULL).  VS_OK, VS_ERR_NOMEM or what the lanes' coefficient sets are refused with; on failure
 * nothing is left allocated.  vs_plan_tables_release frees both arrays. */
typedef struct VsPlanTables {
  double *costab;
  size_t costab_len, taps_off;
  int ltab_entries;
  double *awide;
} VsPlanTables;
int vs_plan_tables_build(const vs_lane *lanes, VsDevLane *dl, size_t n_lanes, const VsBatchStats *st, int filter_only,
                         VsPlanTables *t);
void vs_plan_tables_release(VsPlanTables *t);

/* The launch shape of a plan: which kernel, how many groups and roles per workgroup, which rings.  vs_plan embeds it. */
typedef struct VsPlanShape {
  int group_lanes;   /* utterances per wavefront: VS_WAVE, or VS_NARROW_LANES for periods beyond the 64-column ring */
  unsigned grid;
  int wave_specialised;
  int ws_pairs;      /* groups of 64 utterances per workgroup of the wave-specialised launch */
  int ws_roles;      /* wavefronts per group: 2 or 3 (VsKernelArgs.ws_roles) */
  int ws_layout;     /* VS_WS_LAYOUT_* (VsKernelArgs.ws_layout) */
  int simd_fallback; /* the plan wanted three roles and took two because the wavefronts are not dealt four at a time */
  int ws_shared_simd; /* the wavefronts of a group share a SIMD (grids beyond two groups per CU) */
  int ring_slots;
  int ring_slots_min; /* mixed rings: the shallowest ring of the plan (ring_slots holds the deepest) */
  int ready_min;
  int ltab_entries;
  int ws_pair_bytes; /* LDS bytes of one pair */
  size_t lds_bytes;  /* dynamic LDS of a wave-specialised workgroup's groups (mixed rings: the largest workgroup's sum); one group's ring + cos rows otherwise */
  size_t lds_one_wave; /* ... of one group on the one-wave kernel (source-only kind, cycle log), whatever the fused launch takes */
  int pow_lframe;    /* vowel -n: the frame length all lanes share when the fused kernel takes the frame powers along, else 0 */
  long ondw_pitch;   /* ... frames per row of the noise-width table, 0: no lane asks for output noise */
  size_t flow_pitch; /* wide plans that synthesise: row pitch of the flow between the two kernels */
  int pre1;          /* every lane has pre_emphasis == 1.0 (the reference's default) */
  int wide;          /* some lane carries a coefficient set of 23..40 taps: source kernel -> flow in HBM -> wide filter kernel */
  VsGroupSlot *gmap; /* mixed rings: [n_wg_mixed][4], else NULL; malloc'ed, the caller of vs_plan_shape frees it WHATEVER that returned */
  size_t n_wg_mixed; /* ... its workgroups; stays when gmap has been freed: != 0 says the plan runs over mixed rings */
} VsPlanShape;
/* "are workgroups of `waves` (12 or 8) wavefronts dealt to the SIMDs four at a time?": 1 yes, 0 no or not known */
typedef int (*vs_dealt_fn)(void *user, int waves);
/* Decides the shape from the sorted records (their ready_min is written), the batch's statistics, the CU count (<= 0: 256),
 * the tuning and ltab_entries of the plan's tables.  dealt_fn is asked at most once, and only when the plan has arrived
 * at three roles with more than one group per workgroup and tune->fault is not VS_FAULT_SIMD_DEALING.  VS_OK,
 * VS_ERR_UNSUPPORTED (a period or a batch no ring holds), VS_ERR_NOMEM, VS_ERR_INTERNAL. */
int vs_plan_shape(VsDevLane *dl, size_t n_lanes, size_t n_samples, const VsBatchStats *st, int filter_only, int cu_count,
                  const vs_tuning *tune, int ltab_entries, vs_dealt_fn dealt_fn, void *dealt_user, VsPlanShape *s);

/* what a launch of the plan adds to its shape: from the plan's tuning and the context's arithmetic (VS_ARITH_*) */
typedef struct VsLaunchKnobs {
  int ready_min, gen_min, gen_low, spin_limit, ws_filter_prio; /* the VsKernelArgs fields of these names */
} VsLaunchKnobs;
void vs_plan_knobs(const VsPlanShape *s, const vs_tuning *tune, int arith, VsLaunchKnobs *k);

/* ---- what a launch launches: decided here, looked up and launched by csrc/vs_kernels.hip ---- */
/* A synthesis kernel by name: its family and its template arguments in their order, 0 behind the last.  A family's
 * kernels stand in one file, with their table (csrc/vs_kernel_table.h).
 *   VS_KF_ONE_WAVE, VS_KF_NARROW  vs_synth_kernel<ARITH, KIND, LOG, PRE1> (the narrow build: 16 utterances per wavefront): vs_synth_one_wave.hip
 *   VS_KF_WS, VS_KF_WS_POW        vs_synth_ws_kernel / vs_synth_ws_pow_kernel<ARITH, PRE1, ROLES>: vs_synth_ws.hip
 *   VS_KF_WIDE                    vs_filter_wide_kernel<ARITH>: vs_filter_wide.hip
 *   VS_KF_OUT_POWER, _FILL, VS_KF_OUT_NOISE   vs_out_power_kernel / vs_out_power_fill_kernel / vs_out_noise_kernel<VEC>: vs_out_noise.hip */
enum { VS_KF_ONE_WAVE = 1, VS_KF_NARROW, VS_KF_WS, VS_KF_WS_POW, VS_KF_WIDE, VS_KF_OUT_POWER, VS_KF_OUT_POWER_FILL, VS_KF_OUT_NOISE };
#define VS_KERNEL_ID(family, t0, t1, t2, t3) (((family) << 16) | ((t0) << 12) | ((t1) << 8) | ((t2) << 4) | (t3))
#define VS_KERNEL_FAMILY(id) ((id) >> 16)
/* "vs_synth_ws_kernel<0, true, 3>"; the three vowel -n kernels without their argument */
void vs_kernel_id_name(int id, char *buf, size_t len);

typedef struct VsLaunchPick {
  int kernel;        /* VS_KERNEL_ID */
  unsigned block, grid;
  size_t lds_bytes;  /* dynamic LDS */
} VsLaunchPick;
/* What vs_launch_kernel / vs_launch_kernel_narrow / vs_launch_filter_wide launch when they are given these arguments:
 * 0, or -1 for a launch they refuse (hipErrorInvalidValue). */
int vs_launch_pick(int arith, int kind, bool log, bool wave_specialised, bool pre1, const VsKernelArgs *args, unsigned grid,
                   size_t lds_bytes, VsLaunchPick *pick);
int vs_launch_pick_narrow(int arith, int kind, bool log, bool pre1, unsigned grid, size_t lds_bytes, VsLaunchPick *pick);
int vs_launch_pick_wide(int arith, const VsKernelArgs *args, unsigned grid, VsLaunchPick *pick);
/* ... and vs_launch_out_noise: the power pass (every frame, or the frames the fused kernel left: fill), then the noise pass
 * of segs blocks per row, whose kernel finds its row as ((block * seg_magic) >> 32) >> seg_shift (row_major) or in
 * blockIdx.x.  octets, row_major: VS_ONOISE_OCTETS and VS_ONOISE_ROWMAJOR of the build (shipped: 1, 1). */
typedef struct VsOutNoisePick {
  VsLaunchPick power, noise; /* (noise.grid: row_major, else rows) */
  unsigned noise_grid_y;     /* 1, or segs when not row_major */
  unsigned segs, seg_magic, seg_shift;
} VsOutNoisePick;
int vs_launch_pick_out_noise(const VsKernelArgs *args, int octets, int row_major, VsOutNoisePick *pick);

/* The launches of one vs_plan_launch, in order. */
enum { VS_STEP_KERNEL, VS_STEP_FILTER_WIDE, VS_STEP_OUT_NOISE };
typedef struct VsLaunchStep {
  int what;              /* VS_STEP_*: vs_launch_kernel, vs_launch_filter_wide, vs_launch_out_noise */
  int arith;             /* the context's, as the launchers are given it */
  int kind;              /* VS_STEP_KERNEL: the other selectors of vs_launch_kernel ... */
  bool log, wave_specialised, pre1;
  size_t lds_bytes;      /* ... and the LDS it is given */
  bool awide;            /* the arguments carry the plan's 40-tap sets from here on */
  bool into_flow;        /* this launch only: writes the plan's flow (rows 16-byte aligned) instead of the caller's array, no vowel -n */
  bool from_flow;        /* reads the plan's flow from here on; the cycle log and counts are done with */
  bool pow;              /* takes the frame powers along: the arguments carry odone and pow_lframe from here on */
} VsLaunchStep;
#define VS_PLAN_MAX_STEPS 3
/* log: a cycle log was given (never for the filter kind); onoise: the launch has a noise-width table (the plan's, unless
 * the kind is source-only).  Returns the number of steps. */
int vs_plan_steps(const VsPlanShape *s, int arith, int kind, bool log, bool onoise, VsLaunchStep *steps);

/* the smallest host-to-device copy the runtime hands to a DMA engine instead of a copy kernel (measured: 16 KiB kernel,
 * 64 KiB DMA; tools/overlap_probe.py) */
#define VS_SMALL_BLOCK_MIN ((size_t)65536)
/* Where the parts of a plan lie in its blocks (offsets and sizes in bytes):
 *   a zero-copy plan's one block: records | cos rows + taps | error word | wide taps, zc_bytes in all;
 *   a copying plan's small block: cos rows + taps | group table | error word, small_bytes (>= VS_SMALL_BLOCK_MIN) in all */
typedef struct VsPlanLayout {
  size_t lanes_bytes, cos_bytes, wide_bytes, gmap_bytes; /* what is copied of each part (0: the plan has none) */
  size_t zc_off_cos, zc_off_err, zc_off_wide, zc_bytes;
  size_t small_off_gmap, small_off_err, small_bytes;
} VsPlanLayout;
void vs_plan_layout(size_t n_lanes, size_t costab_len, const VsPlanShape *s, VsPlanLayout *b);
#ifdef __cplusplus
}
#endif
#endif
