/*
 * vs_psola.h -- what the host side (vs_psola_host.c, plain C) and the kernels (vs_psola.hip) of PSOLA share: the per-row
 * record the host uploads, the scratch between the two kernels, the overlap-add kernel's shape, the launch arguments.
 * Also what PSOLA with a time map (vs_psola_ts.h) takes from here: that shape, the launch arguments both have
 * (VsPsCommon) and the host functions both launches call (vs_psola_common_check and its kin).  The device code the two
 * share is vs_psola_dev.h's.
 */
#ifndef VS_PSOLA_H
#define VS_PSOLA_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"

typedef struct VsPsRow { /* one per row */
  int32_t length;
} VsPsRow;               /* 4 bytes */

/* What the plan kernel leaves for the overlap-add kernel next to each vs_psola_mark, [n_lanes][synth_pitch]: the
 * analysis mark a[k] and the two analysis periods of k inside its run (the record alone does not say where the run of k
 * begins and ends). */
typedef struct VsPsAux {
  int32_t a;             /* a[k] */
  int32_t periods;       /* PR(k) | PL(k) << 16, each 1..VS_AC_MAX_LAG */
} VsPsAux;               /* 8 bytes */

/* The overlap-add kernel: a workgroup of VS_PS_BLOCK lanes per (row, tile); a lane makes VS_PS_PER_LANE consecutive
 * samples, one 16-byte piece of the output row.  The tiles are cut where the OUTPUT row's address is a multiple of 16
 * bytes: tile q of a row whose first sample lies `mis` samples behind such an address holds the samples
 * [q*VS_PS_TILE - mis, (q+1)*VS_PS_TILE - mis).  The synthesis marks of a tile are staged VS_PS_STAGE at a time. */
#define VS_PS_BLOCK 256
#define VS_PS_PER_LANE 8
#define VS_PS_TILE (VS_PS_BLOCK * VS_PS_PER_LANE) /* 2048 samples */
#define VS_PS_STAGE 256
#define VS_PS_LDS (VS_PS_STAGE * 16 + 16) /* 4112 bytes, static: t, a, periods and gain of the staged marks; the counters */

/* The launch arguments PSOLA and PSOLA with a time map (vs_psola_ts.h) have in common; vs_psola_common fills them */
typedef struct VsPsCommon {
  const int16_t *pcm;    /* device */
  long pitch;
  long n_lanes;
  const int32_t *marks;
  long marks_pitch;
  const vs_guided_rec *rec;
  const vs_guided_seg *segs; /* NULL: one run per row */
  long seg_pitch;
  const char *start, *period, *gain, *count; /* bytes: strides apply; gain may be NULL */
  int start_stride, period_stride, gain_stride, count_stride;
  long target_pitch;
  int16_t *out;
  long out_pitch;
  vs_psola_stat *stat;
  vs_psola_mark *synth;
  long synth_pitch;
  int pmin, pmax;
} VsPsCommon;

typedef struct VsPsArgs {
  VsPsCommon c;
  long n_samples;
  const VsPsRow *rows;
  VsPsAux *aux;          /* scratch, [n_lanes][synth_pitch] */
} VsPsArgs;

#ifdef __cplusplus
extern "C" {
#endif
/* Device-free (vs_psola_host.c): every refusal of the sizes, strides and options in the order VS_ERR_ARG,
 * VS_ERR_UNSUPPORTED, VS_ERR_RANGE; the row records (VS_ERR_RANGE for a length outside [0, n_samples]); the tiles of a
 * row; the scratch. */
int vs_psola_check(const vs_psola_opts *opts, size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch,
                   int has_segs, size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain,
                   size_t gain_stride, size_t count_stride, size_t target_pitch, size_t out_pitch, size_t synth_pitch,
                   vs_psola_opts *resolved);
int vs_psola_fill(const int32_t *lengths, size_t n_lanes, size_t n_samples, VsPsRow *rows);
/* What PSOLA and PSOLA with a time map (vs_psola_ts_host.c) do alike, device-free too.  common_check: what both checks
 * refuse, the first of VS_ERR_ARG, VS_ERR_UNSUPPORTED, VS_ERR_RANGE -- each check puts its own refusals of a kind in
 * front of the later kinds; out_samples: the output row's samples (PSOLA: n_samples).  bad_pointers: a pointer either
 * launch needs is NULL or one is not aligned to its element.  common: the launch arguments both have.  parts: the first
 * seven parts of either host-buffer call (struct VsHostPart: vs_internal.h). */
int vs_psola_common_check(size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch, int has_segs,
                          size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain, size_t gain_stride,
                          size_t count_stride, size_t target_pitch, size_t out_pitch, size_t out_samples,
                          size_t synth_pitch, int pmin, int pmax);
int vs_psola_bad_pointers(const vs_ctx *ctx, const int16_t *pcm_dev, const int32_t *marks_dev,
                          const vs_guided_rec *rec_dev, const vs_guided_seg *segs_dev, const int32_t *start_dev,
                          const int32_t *period_dev, const int32_t *gain_dev, const int32_t *count_dev,
                          const int16_t *out_dev, const vs_psola_stat *stat_dev, const vs_psola_mark *synth_dev);
void vs_psola_common(VsPsCommon *c, int pmin, int pmax, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                     const int32_t *marks_dev, size_t marks_pitch, const vs_guided_rec *rec_dev,
                     const vs_guided_seg *segs_dev, size_t seg_pitch, const int32_t *start_dev, size_t start_stride,
                     const int32_t *period_dev, size_t period_stride, const int32_t *gain_dev, size_t gain_stride,
                     const int32_t *count_dev, size_t count_stride, size_t target_pitch, int16_t *out_dev,
                     size_t out_pitch, vs_psola_stat *stat_dev, vs_psola_mark *synth_dev, size_t synth_pitch);
struct VsHostPart;
void vs_psola_parts(struct VsHostPart *parts, size_t n_lanes, const int32_t *marks, size_t marks_pitch,
                    const vs_guided_rec *rec, const vs_guided_seg *segs, size_t seg_pitch, const int32_t *start,
                    const int32_t *period, const int32_t *gain, const int32_t *count, size_t target_pitch);
size_t vs_psola_tiles(size_t n_samples);
size_t vs_psola_scratch_bytes(size_t n_lanes, size_t synth_pitch);
/* launcher (vs_psola.hip): the plan kernel, one lane per row; the overlap-add kernel behind it */
hipError_t vs_launch_psola(const VsPsArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
