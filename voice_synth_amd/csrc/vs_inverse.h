/*
 * vs_inverse.h -- what the host side (vs_inverse_host.c, plain C) and the kernels (vs_inverse.hip) of the inverse filter
 * share: the launch arguments.  The lanes per workgroup, the two window classes and the LDS plan of the glide kernels
 * are the coefficient tracks' (vs_track.h): the same row selects the same taps at the same sample in both.
 */
#ifndef VS_INVERSE_H
#define VS_INVERSE_H

#include "vs_track.h"

typedef struct VsInverseArgs {
  const int16_t *in;
  int16_t *out;
  long in_pitch, out_pitch;  /* samples */
  long n_lanes;
  const vs_inverse_row *rows; /* device, one per row */
  const double *coefs;        /* [n_lanes][sets_pitch][order + 1] */
  vs_inverse_stat *stat;      /* [n_lanes] or NULL */
  long sets_pitch;
  int order;
  int vec_ok;                 /* 1: every row start is 4-byte aligned, 16-byte vector loads and stores allowed */
} VsInverseArgs;

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_inverse.hip): arith VS_ARITH_EXACT or anything else (the FMA form), mode VS_TRACK_HOLD / VS_TRACK_GLIDE */
hipError_t vs_launch_inverse(int arith, int mode, const VsInverseArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
