/*
 * vs_lpc.h -- what the host side (vs_lpc_host.c, plain C) and the kernel (vs_lpc.hip) of the LPC analysis share: the
 * per-row record the host uploads, the launch arguments, the frame block and LDS plan of the kernel.
 */
#ifndef VS_LPC_H
#define VS_LPC_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"

#if defined(__HIPCC__)
#define VS_LPC_HD __host__ __device__
#else
#define VS_LPC_HD
#endif

typedef struct VsLpcRow { /* one per row, built by the host from fs / lengths / the options */
  int64_t first;          /* index of the row's frame 0 among all frames of the call (prefix sum of n_frames) */
  int32_t fs, L, H;       /* rate, window and hop in samples (H unused with one centre frame) */
  int32_t s0;             /* start of frame 0 */
  int32_t n_frames;
  int32_t woff;           /* the row's window table: windows[woff .. woff + L) */
} VsLpcRow;               /* 32 bytes */

typedef struct VsLpcArgs {
  const int16_t *pcm;
  long pitch;             /* samples */
  long n_lanes;
  long total_frames;      /* sum of n_frames */
  const VsLpcRow *rows;   /* device */
  const int32_t *windows; /* device */
  vs_lpc_frame *frames;
  double *formants;       /* NULL: none */
  double *coefs;          /* NULL: none */
  long frames_pitch;
  int order, pre, n_formants;
  double f_lo;
} VsLpcArgs;

/* The kernel: 256 threads take VS_LPC_FB(order) consecutive frames of the call (across rows).  A thread owns one
 * (frame, group of four adjacent lags); samples go through LDS in chunks of VS_LPC_CHUNK per frame. */
#define VS_LPC_THREADS 256
#define VS_LPC_CHUNK 64
static inline VS_LPC_HD int vs_lpc_groups(int order) { return (order + 1 + 3) / 4; }
static inline VS_LPC_HD int vs_lpc_fb(int order)
{
  const int fb = VS_LPC_THREADS / vs_lpc_groups(order);
  return fb < 64 ? fb : 64;
}
/* LDS row of one frame's chunk, in doubles: VS_LPC_CHUNK + 4G - 1 values, odd (b64 reads of 32 lanes on distinct banks) */
static inline VS_LPC_HD int vs_lpc_stride(int order) { return (VS_LPC_CHUNK + 4 * vs_lpc_groups(order) - 1) | 1; }
/* dynamic LDS in doubles: the chunk rows, or r and a of every frame ([order+1][FB] each), whichever is larger */
static inline VS_LPC_HD int vs_lpc_lds_doubles(int order)
{
  const int stage = vs_lpc_fb(order) * vs_lpc_stride(order), ra = 2 * (order + 1) * vs_lpc_fb(order);
  return stage > ra ? stage : ra;
}

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_lpc.hip): grid from total_frames and the order; nothing is launched for 0 frames */
hipError_t vs_launch_lpc(const VsLpcArgs *args, hipStream_t stream);
#ifndef __HIPCC__
/* Host side (vs_lpc_host.c), for the launches that run on vs_lpc's frames (vs_lpc_launch, vs_iaif_launch): the checks
 * of vs_lpc_launch, every row's frames, the window tables, the upload of both through the slot; *args filled but for
 * what the caller adds, *blk to be retired behind the caller's kernel (vs_rec_retire).  opts is not NULL. */
struct VsRecSlot;
struct VsRecBlock;
int vs_lpc_rows_upload(vs_ctx *ctx, struct VsRecSlot *slot, const vs_lpc_opts *opts, const int16_t *pcm_dev, size_t pitch,
                       size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                       vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev, struct VsRecBlock *blk,
                       VsLpcArgs *args);
int vs_lpc_check_opts(const vs_lpc_opts *opts); /* VS_OK, VS_ERR_ARG or VS_ERR_RANGE, as vs_lpc_launch answers */
#endif
#ifdef __cplusplus
}
#endif

#endif
