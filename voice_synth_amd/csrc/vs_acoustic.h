/*
 * vs_acoustic.h -- what the host side (vs_acoustic_host.c, plain C) and the kernels (vs_acoustic.hip) of the acoustic
 * measurement share: the per-row record the host uploads, the launch arguments, the LDS plan of the period kernel.
 */
#ifndef VS_ACOUSTIC_H
#define VS_ACOUSTIC_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"

#if defined(__HIPCC__)
#define VS_AC_HD __host__ __device__
#else
#define VS_AC_HD
#endif

typedef struct VsAcRow { /* one per row, built by the host from fs / lengths / the options */
  int32_t len, fs, tmin, tmax;
} VsAcRow;

typedef struct VsAcArgs {
  const int16_t *pcm;
  long pitch;          /* samples */
  long n_lanes;
  long n_samples;
  const VsAcRow *rows; /* device */
  vs_acoustic *out;
  int32_t *marks;      /* NULL: none */
  long marks_pitch;
  int polarity;
} VsAcArgs;

/* LDS of the period kernel, in doubles: the window (3*tmax + 2 samples, rounded up, and 4 zeros past it for the last
 * group of lags), the partial sums [S][4G] (at most max(4G, 1024)), the block reduction (8) */
static inline VS_AC_HD int vs_ac_xs_doubles(int tmax) { return ((3 * tmax + 2 + 4) + 3) & ~3; }
static inline VS_AC_HD int vs_ac_rp_doubles(int tmin, int tmax)
{
  const int nl = tmax + 3 - tmin, G = (nl + 3) / 4;
  const int S = G >= 256 ? 1 : 256 / G;
  return 4 * G * S;
}
static inline VS_AC_HD int vs_ac_lds_doubles(int tmin, int tmax)
{
  return vs_ac_xs_doubles(tmax) + vs_ac_rp_doubles(tmin, tmax) + 8;
}

#ifdef __cplusplus
extern "C" {
#endif
/* launchers (vs_acoustic.hip): grid / LDS from the arguments; lds_doubles = max over the rows of vs_ac_lds_doubles */
hipError_t vs_launch_measure(const VsAcArgs *args, int lds_doubles, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
