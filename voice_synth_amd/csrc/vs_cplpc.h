/*
 * vs_cplpc.h -- what the host side (vs_cplpc_host.c, plain C) and the kernel (vs_cplpc.hip) of the closed-phase
 * covariance LPC share: the launch arguments, the staging chunk and the LDS plan of the kernel.  The per-row record is
 * the LPC analysis's (VsLpcRow: first, fs, L, H, s0, n_frames); with window_s == 0 a row has one frame that spans it.
 */
#ifndef VS_CPLPC_H
#define VS_CPLPC_H

#include "vs_lpc.h"

typedef struct VsCplpcArgs {
  VsLpcArgs lpc;                   /* pcm, pitch, n_lanes, total_frames, rows, frames, formants, coefs, frames_pitch, order,
                                      n_formants, f_lo; windows and pre are not read */
  const vs_glottal_rec *glottal;   /* [n_lanes] */
  const vs_glottal_cycle *cycles;  /* [n_lanes][cycles_pitch] */
  long cycles_pitch;
  int32_t *counts;                 /* [n_lanes][frames_pitch][2] or NULL */
  int anchor, delay, span_q, min_equations;
} VsCplpcArgs;

/* The kernel: one wavefront per frame.  The equations of a span go through LDS in chunks of VS_CPLPC_CHUNK, each with
 * the order samples in front of it, counted from the span's first equation (not from the row's start). */
#define VS_CPLPC_THREADS 64
#define VS_CPLPC_CHUNK 256
/* stride of the covariance triangle in doubles: odd and > order, so that a column and a row are both read without a
 * bank conflict */
static inline VS_LPC_HD int vs_cplpc_stride(int order) { return (order + 2) | 1; }
/* dynamic LDS in bytes: the triangle [order+1][stride] of doubles; next to it the kernel has 1752 bytes of static LDS
 * (the chunk, the taps for the root phase, the frame's words).  Order 22: 4600 + 1752; order 40: 14104 + 1752 */
static inline VS_LPC_HD int vs_cplpc_lds_bytes(int order) { return (order + 1) * vs_cplpc_stride(order) * 8; }
#define VS_CPLPC_LDS_STATIC 1752

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_cplpc.hip): one workgroup per frame; nothing is launched for 0 frames */
hipError_t vs_launch_cplpc(const VsCplpcArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
