/*
 * vs_track.h -- what the host side (vs_track_host.c, plain C) and the kernels (vs_track.hip) of the coefficient tracks
 * share: the launch arguments, the window classes and the LDS plan of the glide kernels.
 */
#ifndef VS_TRACK_H
#define VS_TRACK_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"

#if defined(__HIPCC__)
#define VS_TRACK_HD __host__ __device__
#else
#define VS_TRACK_HD
#endif

typedef struct VsTrackArgs {
  const int16_t *in;
  int16_t *out;
  long in_pitch, out_pitch;  /* samples */
  long n_lanes;
  const vs_track_row *rows;  /* device, one per row */
  const double *coefs;       /* [n_lanes][sets_pitch][order + 1] */
  const double *gains;       /* [n_lanes][sets_pitch] or NULL */
  vs_track_stat *stat;       /* [n_lanes] or NULL */
  long sets_pitch;
  int order;
  int vec_ok;                /* 1: every row start is 4-byte aligned, 16-byte vector loads and stores allowed */
} VsTrackArgs;

/* One row per lane, 64-lane workgroups.  Two window classes: orders up to VS_TRACK_P0 on a window of VS_TRACK_GROUP
 * doubles, the others on 2 * VS_TRACK_GROUP (a set may change at either half). */
#define VS_TRACK_LANES 64
#define VS_TRACK_P0 22
#define VS_TRACK_P1 40
static inline VS_TRACK_HD int vs_track_class_order(int order) { return order <= VS_TRACK_P0 ? VS_TRACK_P0 : VS_TRACK_P1; }
/* glide: ka and kb of every lane, [2][P][64] doubles ([slot][i][lane]: the lanes of a b64 access are consecutive) */
static inline VS_TRACK_HD int vs_track_lds_doubles(int order) { return 2 * vs_track_class_order(order) * VS_TRACK_LANES; }

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_track.hip): arith VS_ARITH_EXACT or anything else (the FMA form), mode VS_TRACK_HOLD / VS_TRACK_GLIDE */
hipError_t vs_launch_track(int arith, int mode, const VsTrackArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
