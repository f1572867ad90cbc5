/*
 * vs_iaif.h -- what the host side (vs_iaif_host.c, plain C) and the kernel (vs_iaif.hip) of the IAIF analysis share: the
 * launch arguments and the LDS plan of the kernel.  The frames, the per-row records and the window tables are those of
 * the LPC analysis (vs_lpc.h).
 */
#ifndef VS_IAIF_H
#define VS_IAIF_H

#include "vs_lpc.h"

typedef struct VsIaifArgs {
  VsLpcArgs lpc;   /* pre is 0; order = p, the vocal-tract order; coefs = V2 */
  double *glottal; /* c2, [n_lanes][frames_pitch][glottal_order + 1]; NULL: none */
  int glottal_order;
  double leak;
} VsIaifArgs;

/* The kernel: vs_lpc's frame block, 256 threads on VS_LPC_FB(p) consecutive frames of the call, a thread per (frame,
 * group of four adjacent lags).  Per frame and chunk of VS_LPC_CHUNK samples LDS holds
 *   V: the windowed stage signal as doubles, H = 4G - 1 values of the chunk before and the chunk: vs_lpc's row
 *      (vs_lpc_stride(p) doubles); r and a of the recursion lie over it between the stages, as in vs_lpc;
 *   E: the input as int16, the p samples before the chunk and the chunk;
 *   T: the taps of the stage's FIR, at most p doubles. */
static inline VS_LPC_HD int vs_iaif_estride(int order) { return (VS_LPC_CHUNK + order + 1) & ~1; } /* int16, even */
static inline VS_LPC_HD int vs_iaif_tstride(int order) { return order | 1; }
static inline VS_LPC_HD int vs_iaif_e_doubles(int order) { return (vs_lpc_fb(order) * vs_iaif_estride(order) + 3) / 4; }
static inline VS_LPC_HD int vs_iaif_lds_doubles(int order)
{
  return vs_lpc_lds_doubles(order) + vs_iaif_e_doubles(order) + vs_lpc_fb(order) * vs_iaif_tstride(order);
}

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_iaif.hip): grid from total_frames and the order; nothing is launched for 0 frames */
hipError_t vs_launch_iaif(const VsIaifArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
