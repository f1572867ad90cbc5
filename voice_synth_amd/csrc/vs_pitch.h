/*
 * vs_pitch.h -- what the host side (vs_pitch_host.c, plain C) and the kernels (vs_pitch.hip) of the pitch track share:
 * the per-row record the host uploads, the launch arguments, the LDS plans of the two kernels.
 */
#ifndef VS_PITCH_H
#define VS_PITCH_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_acoustic.h"

typedef struct VsPtRow { /* one per row, built by the host from fs / lengths / the options */
  int64_t first;         /* index of the row's frame 0 among all frames of the call (prefix sum of n_frames) */
  int32_t len, fs, tmin, tmax;
  int32_t H, n_frames;
} VsPtRow;               /* 32 bytes */

typedef struct VsPtArgs {
  const int16_t *pcm;
  long pitch;            /* samples */
  long n_lanes;
  long total_frames;     /* sum of n_frames */
  const VsPtRow *rows;   /* device */
  const int32_t *lg;     /* device: Lg[0 .. VS_AC_MAX_LAG], behind the rows in the same block */
  vs_pitch_frame *frames;
  long frames_pitch;
  int voicing_q, octave_q, jump_q, vuv_q, silence_rms;
} VsPtArgs;

/* The candidate kernel: VS_AC_A_THREADS (256) threads per frame.  Dynamic LDS in doubles: the period kernel's window and
 * partial sums (vs_acoustic.h: 3*tmax + 2 samples and 4 zeros; [S][4G], which the selection keys overlay as ints once
 * r(t) is used up), e(t) of every lag, the block reduction and scan (8 + 8), q(t) of every lag as ints.  The largest,
 * tmax 2048 with tmin 2: 6152 + 2052 + 2052 + 16 + 1026 doubles = 90384 bytes, one workgroup on a CU; at 16 kHz with the
 * defaults (tmax 320) 18384 bytes, eight. */
static inline VS_AC_HD int vs_pt_lags(int tmin, int tmax) { return tmax + 3 - tmin; }         /* tmin-1 .. tmax+1 */
static inline VS_AC_HD int vs_pt_e_doubles(int tmin, int tmax) { return (vs_pt_lags(tmin, tmax) + 3) & ~3; }
static inline VS_AC_HD int vs_pt_lds_doubles(int tmin, int tmax)
{
  return vs_ac_xs_doubles(tmax) + vs_ac_rp_doubles(tmin, tmax) + vs_pt_e_doubles(tmin, tmax) + 16 +
         vs_pt_e_doubles(tmin, tmax) / 2;
}
/* The path kernel: one wavefront per row; static LDS: the Lg table */
#define VS_PT_PATH_LDS ((VS_AC_MAX_LAG + 1) * 4)

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_pitch.hip): the candidate kernel over total_frames, the path kernel over the rows; lds_doubles = max over
 * the rows of vs_pt_lds_doubles; nothing is launched for 0 frames */
hipError_t vs_launch_pitch(const VsPtArgs *args, int lds_doubles, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
