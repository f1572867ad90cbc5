/*
 * vs_glottal.h -- what the host side (vs_glottal_host.c, plain C) and the kernel (vs_glottal.hip) of the glottal
 * parameters share: the launch arguments.  There is no per-row record: the kernel reads the measurement's own.
 */
#ifndef VS_GLOTTAL_H
#define VS_GLOTTAL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"

typedef struct VsGlArgs {
  const int16_t *pcm;
  long pitch;              /* samples */
  long n_lanes;
  int n_samples;
  int marks_pitch;
  const vs_acoustic *meas; /* device, written by vs_launch_measure */
  const int32_t *marks;    /* device, [n_lanes][marks_pitch] */
  vs_glottal_rec *out;
  vs_glottal_cycle *cycles; /* NULL: none */
  long cycles_pitch;
  int level_open, level_mid, polarity;
} VsGlArgs;

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_glottal.hip): one wavefront per row */
hipError_t vs_launch_glottal(const VsGlArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
