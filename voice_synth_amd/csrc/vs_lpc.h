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
/* Host side (vs_lpc_host.c), for the launches that run on vs_lpc's frames (vs_lpc_launch, vs_iaif_launch,
 * vs_cplpc_launch): the checks of vs_lpc_launch, every row's frames, the window tables, the upload of both through the
 * slot; *args filled but for what the caller adds, *blk to be retired behind the caller's kernel (vs_rec_retire).  opts
 * is not NULL.  whole (vs_cplpc_launch with window_s == 0, which the other two refuse): every row's record is
 * vs_lpc_row_whole's instead, first = the row's index, and there are no window tables: args->windows is NULL. */
struct VsRecSlot;
struct VsRecBlock;
struct VsHostPart;
int vs_lpc_rows_upload(vs_ctx *ctx, struct VsRecSlot *slot, const vs_lpc_opts *opts, int whole, const int16_t *pcm_dev,
                       size_t pitch, size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths,
                       size_t frames_pitch, vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev,
                       struct VsRecBlock *blk, VsLpcArgs *args);
/* one frame over the whole row: fs, L = len, n_frames = 1, everything else 0; VS_ERR_RANGE for fs <= 0 or len < 0 */
int vs_lpc_row_whole(int32_t fs, int32_t len, VsLpcRow *r);
int vs_lpc_check_opts(const vs_lpc_opts *opts); /* VS_OK, VS_ERR_ARG or VS_ERR_RANGE, as vs_lpc_launch answers */
/* What the launches and host-buffer calls of the three analyses check alike before they look at their options:
 * VS_ERR_ARG, then the 2^31 limits (VS_ERR_UNSUPPORTED).  need_frames_pitch: frames_pitch == 0 is VS_ERR_ARG too (the
 * host-buffer calls and vs_cplpc_launch; vs_lpc_launch and vs_iaif_launch answer VS_ERR_RANGE for a row with a frame) */
int vs_frame_check(const vs_ctx *ctx, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
                   const int32_t *fs, size_t frames_pitch, const vs_lpc_frame *frames, int need_frames_pitch);
/* the parts of a host-buffer call every analysis has: parts[0..2] = the records, the formants, the coefficients of
 * n_lanes * frames_pitch = nfr frames, up and back (what no frame covers comes back as it went) */
void vs_frame_parts(struct VsHostPart *parts, size_t nfr, int order, int n_formants, vs_lpc_frame *frames,
                    double *formants, double *coefs);
/* o = the caller's options, or the defaults for NULL */
#define VS_OPTS_OR(o, opts, defaults) ((opts) ? (void)((o) = *(opts)) : (void)defaults(&(o)))
#endif
#ifdef __cplusplus
}
#endif

#endif
