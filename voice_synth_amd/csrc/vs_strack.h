/*
 * vs_strack.h -- what the host side (vs_strack_host.c, plain C) and the kernel (vs_strack.hip) of the source track
 * share: the per-row record the host uploads, the layout of the uploaded block, the launch arguments.
 */
#ifndef VS_STRACK_H
#define VS_STRACK_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"

#define VS_STF_JITTER 0x1u  /* VS_FLAG_JITTER and jitter != 0 */
#define VS_STF_SHIMMER 0x2u /* VS_FLAG_SHIMMER and shimmer != 0 */
#define VS_STF_NOISE 0x4u   /* VS_FLAG_NOISE */

typedef struct VsStRow { /* one per row, built by the host from the lane and the vs_strack_row */
  float jitter, shimmer, K, Kvar;
  float DC, noise, cq;
  int32_t amp;
  uint32_t flags, key0, key1;
  int32_t dcs;           /* (short)DC */
  int32_t n_frames, hop, offset, length;
  int32_t pmin, pmax, reserved_[2];
} VsStRow;               /* 80 bytes */

/* The longest cycle: T <= (float)1.2 * VS_AC_MAX_LAG = 2457, and the pulse reaches 2*T2 <= VS_AC_MAX_LAG + 2 (cq = 1).
 * The kernel keeps one cycle (int16) and, with a cycle log, its noise values (int16) in LDS. */
#define VS_ST_CYCLE_MAX 2560
#define VS_ST_LDS (2 * VS_ST_CYCLE_MAX * 2) /* 10240 bytes, static */

/* T2 of a period: ceil(0.5 * cq * P), flowgen_shimmer.c:317 */
#define VS_ST_T2_MAX (VS_AC_MAX_LAG / 2 + 1)

/* The uploaded block: [n_lanes] VsStRow, then toff int32 [VS_ST_T2_MAX + 1] (the offset of T2's cos row in doubles, -1: no
 * row of the call reaches that T2) padded to a multiple of 8 bytes, then the cos rows, T2 doubles each. */
typedef struct VsStPlan {
  size_t toff_at;      /* bytes from the block's start */
  size_t cos_at;
  size_t cos_entries;  /* doubles */
  size_t bytes;        /* of the whole block */
} VsStPlan;

typedef struct VsStArgs {
  const VsStRow *rows;   /* device */
  const int32_t *toff;
  const double *costab;
  const char *period;    /* bytes: strides apply */
  const char *amp;       /* NULL: the lane's amp */
  int period_stride, amp_stride;
  long frames_pitch;
  int16_t *out;
  long out_pitch;
  vs_strack_stat *stat;
  vs_strack_cycle *cycles; /* NULL: no log */
  long n_lanes;
  int cycles_pitch;
  int max_reject;
} VsStArgs;

#ifdef __cplusplus
extern "C" {
#endif
/* Device-free (vs_strack_host.c): the option checks and the row plan.  check: every VS_ERR_ARG of the sizes and strides,
 * then VS_ERR_UNSUPPORTED, then the options.  plan: the lanes' and rows' refusals, which T2 are needed
 * (need[T2] for T2 in [0, VS_ST_T2_MAX]) and the block's layout.  fill: the records, toff and the cos rows into a block
 * of plan->bytes. */
int vs_strack_check(const vs_strack_opts *opts, size_t n_lanes, size_t n_samples, size_t period_stride,
                    size_t frames_pitch, int has_amp, size_t amp_stride, size_t out_pitch, int has_cycles,
                    size_t cycles_pitch, vs_strack_opts *resolved);
int vs_strack_plan(const vs_lane *lanes, const vs_strack_row *rows, size_t n_lanes, size_t n_samples, size_t frames_pitch,
                   uint8_t *need, VsStPlan *plan);
void vs_strack_fill(const vs_lane *lanes, const vs_strack_row *rows, size_t n_lanes, const uint8_t *need,
                    const VsStPlan *plan, void *block);
/* launcher (vs_strack.hip): one wavefront per row */
hipError_t vs_launch_strack(const VsStArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
