/*
 * vs_guided.h -- what the host side (vs_guided_host.c, plain C) and the kernels (vs_guided.hip) of the guided marks
 * share: the per-row record the host uploads, the plan kernel's scratch, the launch arguments.
 */
#ifndef VS_GUIDED_H
#define VS_GUIDED_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"

typedef struct VsMgRow { /* one per row, built by the host from fs / lengths / the options */
  int32_t len, fs, tmin, tmax;
  int32_t H, n_frames, C, reserved_;
} VsMgRow;               /* 32 bytes */

typedef struct VsMgHead { /* one per row, written by the plan kernel for the walk kernel */
  int64_t Q;              /* sum of clamp(q, 0, 32768) over the frames of the walked runs */
  int32_t nF;             /* ... and their count */
  int32_t first;          /* first frame of the first walked run; n_frames without one */
} VsMgHead;               /* 16 bytes */

/* The plan kernel's scratch, [n_lanes][frames_pitch] each, lent by the context's retired-block cache:
 *   lag[f]  = the lag of frame f if it lies in a walked run, else 0
 *   link[f] = the last frame of its run if it does; else the first frame of the next walked run (n_frames: none) */
typedef struct VsMgArgs {
  const int16_t *pcm;
  long pitch;            /* samples */
  long n_lanes;
  long n_samples;
  const VsMgRow *rows;   /* device */
  const vs_pitch_frame *frames;
  long frames_pitch;
  VsMgHead *head;        /* [n_lanes] */
  int32_t *lag, *link;
  vs_acoustic *out;
  int32_t *marks;        /* NULL: none */
  long marks_pitch;
  vs_guided_rec *rec;
  vs_guided_seg *segs;   /* NULL: none */
  long seg_pitch;
  int polarity, segments, edge_frames, min_frames;
} VsMgArgs;

/* bytes of scratch behind one launch: the heads, then lag and link */
static inline size_t vs_mg_scratch_bytes(size_t n_lanes, size_t frames_pitch)
{
  return n_lanes * sizeof(VsMgHead) + 2 * n_lanes * frames_pitch * sizeof(int32_t);
}

/* The walk kernel: 64 rows per workgroup (one wavefront), [64 x VS_MG_TILE] int16 tiles with an odd-dword row stride:
 * its static LDS.  The plan kernel (one wavefront per row) has none. */
#define VS_MG_TILE 128
#define VS_MG_PAD 2
#define VS_MG_WALK_LDS (64 * (VS_MG_TILE + VS_MG_PAD) * 2) /* 16640 bytes */

#ifdef __cplusplus
extern "C" {
#endif
/* launcher (vs_guided.hip): the plan kernel over the rows, the walk kernel over groups of 64 rows */
hipError_t vs_launch_guided(const VsMgArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
