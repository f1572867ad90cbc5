/*
 * vs_psola_ts.h -- what the host side (vs_psola_ts_host.c, plain C) and the kernels (vs_psola_ts.hip) of PSOLA with a
 * time map share: the per-row record the host uploads, the scratch between the two kernels, the launch arguments.  The
 * overlap-add kernel's shape -- VS_PS_BLOCK lanes, VS_PS_PER_LANE samples a lane, tiles of VS_PS_TILE samples cut at the
 * OUTPUT row's 16-byte addresses, VS_PS_STAGE marks staged at a time -- is PSOLA's (vs_psola.h), and so are the launch
 * arguments the two have in common (VsPsCommon) and the refusals, pointer checks and host parts behind them, which
 * vs_psola_ts_host.c calls in vs_psola_host.c.
 */
#ifndef VS_PSOLA_TS_H
#define VS_PSOLA_TS_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_psola.h"

typedef struct VsPtRow { /* one per row */
  int32_t length;        /* of the input row */
  int32_t len_out;       /* of the output row */
} VsPtRow;               /* 8 bytes */

/* What the plan kernel leaves for the overlap-add kernel next to each vs_psola_mark, [n_lanes][synth_pitch]: the
 * analysis mark of the record's left grain and of its right grain (they differ at a boundary behind a stretch without
 * marks) and the two analysis periods, PR of the left grain's stretch and PL of the right grain's. */
typedef struct VsPtAux {
  int32_t a_left;        /* b[k] of the stretch behind the mark */
  int32_t a_right;       /* b[k] of the stretch before it */
  int32_t periods;       /* PR | PL << 16, each 1..VS_AC_MAX_LAG */
} VsPtAux;               /* 12 bytes */

#define VS_PT_LDS (VS_PS_STAGE * 20 + 16) /* 5136 bytes, static: t, both marks, periods and gain of the staged marks; the counters */

typedef struct VsPtArgs {
  VsPsCommon c;
  long out_samples;
  const VsPtRow *rows;
  const vs_psola_anchor *map;
  const int32_t *map_count;
  long map_pitch;
  VsPtAux *aux;          /* scratch, [n_lanes][synth_pitch] */
  int unvoiced;
} VsPtArgs;

#ifdef __cplusplus
extern "C" {
#endif
/* Device-free (vs_psola_ts_host.c): every refusal of the sizes, strides and options in the order VS_ERR_ARG,
 * VS_ERR_UNSUPPORTED, VS_ERR_RANGE; whether two batches of int16 rows share a byte; the row records (VS_ERR_RANGE for a
 * length outside [0, n_samples] or an output length outside [0, out_samples]); the scratch. */
int vs_psola_ts_check(const vs_psola_ts_opts *opts, size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch,
                      int has_segs, size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain,
                      size_t gain_stride, size_t count_stride, size_t target_pitch, size_t map_pitch, size_t out_pitch,
                      size_t out_samples, size_t synth_pitch, vs_psola_ts_opts *resolved);
int vs_psola_ts_overlap(const void *a, size_t a_pitch, size_t a_samples, const void *b, size_t b_pitch, size_t b_samples,
                        size_t n_lanes);
int vs_psola_ts_fill(const int32_t *lengths, const int32_t *out_lengths, size_t n_lanes, size_t n_samples,
                     size_t out_samples, VsPtRow *rows);
size_t vs_psola_ts_scratch_bytes(size_t n_lanes, size_t synth_pitch);
/* launcher (vs_psola_ts.hip): the plan kernel, one lane per row; the overlap-add kernel behind it */
hipError_t vs_launch_psola_ts(const VsPtArgs *args, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
