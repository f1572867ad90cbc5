/*
 * vs_inverse_host.c -- host side of the inverse filter (include/voice_synth.h, "inverse filtering"): validation, the
 * upload of the per-row records, the kernels of vs_inverse.hip, and the row that runs over vs_lpc's frames.
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.
 */
#include <math.h>
#include <string.h>

#include "vs_inverse.h"
#include "vs_internal.h"

int vs_inverse_from_lpc(const vs_lpc_opts *opts, int32_t fs, int32_t len, int mode, vs_inverse_row *row)
{
  vs_track_row t;
  if (!row) return VS_ERR_ARG;
  const int rc = vs_track_from_lpc(opts, fs, len, mode, &t); /* the same sets at the same samples */
  if (rc != VS_OK) return rc;
  row->n_sets = t.n_sets;
  row->hop = t.hop;
  row->offset = t.offset;
  row->length = t.length;
  row->scale = 1.0f;
  row->de_emphasis = 0.0f;
  return VS_OK;
}

/* what vs_track checks of a call and its rows, then de_emphasis and scale of every row */
static int check_call(int mode, int order, size_t in_pitch, size_t out_pitch, size_t n_lanes, size_t n_samples,
                      const vs_inverse_row *rows, size_t sets_pitch)
{
  const int rc = vs_setwalk_check(mode, order, in_pitch, out_pitch, n_lanes, n_samples, sets_pitch, &rows->n_sets,
                                  &rows->hop, &rows->length, sizeof(*rows));
  if (rc != VS_OK) return rc;
  for (size_t i = 0; i < n_lanes; i++) /* (written so that a NaN fails) */
    if (!(rows[i].de_emphasis >= 0.0f && rows[i].de_emphasis <= 1.0f) || !isfinite(rows[i].scale)) return VS_ERR_RANGE;
  return VS_OK;
}

int vs_inverse_launch(vs_ctx *ctx, int mode, int order, const int16_t *pcm_dev, size_t in_pitch, int16_t *out_dev,
                      size_t out_pitch, size_t n_lanes, size_t n_samples, const vs_inverse_row *rows,
                      const double *coefs_dev, size_t sets_pitch, vs_inverse_stat *stat_dev)
{
  if (!ctx || !pcm_dev || !out_dev || !rows || !coefs_dev) return VS_ERR_ARG;
  int rc = check_call(mode, order, in_pitch, out_pitch, n_lanes, n_samples, rows, sets_pitch);
  if (rc != VS_OK) return rc;

  const size_t bytes = n_lanes * sizeof(vs_inverse_row);
  void *host = NULL;
  VsRecBlock blk;
  rc = vs_rec_stage(ctx, &ctx->rec_inverse, bytes, &host);
  if (rc != VS_OK) return rc;
  memcpy(host, rows, bytes);
  rc = vs_rec_upload(ctx, &ctx->rec_inverse, bytes, &blk);
  if (rc != VS_OK) return rc;
  VsInverseArgs a;
  memset(&a, 0, sizeof(a));
  a.in = pcm_dev;
  a.out = out_dev;
  a.in_pitch = (long)in_pitch;
  a.out_pitch = (long)out_pitch;
  a.n_lanes = (long)n_lanes;
  a.rows = (const vs_inverse_row *)blk.dev;
  a.coefs = coefs_dev;
  a.stat = stat_dev;
  a.sets_pitch = (long)sets_pitch;
  a.order = order;
  a.vec_ok = vs_vec_ok(pcm_dev, in_pitch, out_dev, out_pitch);
  return vs_rec_retire(ctx, &blk, vs_launch_inverse(ctx->arith, mode, &a, ctx->stream));
}

int vs_inverse(vs_ctx *ctx, int mode, int order, const int16_t *pcm, int16_t *flow, size_t n_lanes, size_t n_samples,
               const vs_inverse_row *rows, const double *coefs, size_t sets_pitch, vs_inverse_stat *stat)
{
  if (!ctx || !pcm || !flow || !rows || !coefs) return VS_ERR_ARG;
  int rc = check_call(mode, order, n_samples, n_samples, n_lanes, n_samples, rows, sets_pitch);
  if (rc != VS_OK) return rc;
  /* the speech in d_in; the flow goes up and comes back (what lies past a row's length comes back as it went), the sets
   * go up, the status records come back */
  const size_t pcm_bytes = n_lanes * n_samples * sizeof(int16_t);
  VsHostPart parts[3] = {{flow, pcm_bytes, VS_PART_UP | VS_PART_DOWN, NULL},
                         {(void *)coefs, n_lanes * sets_pitch * (size_t)(order + 1) * sizeof(double), VS_PART_UP, NULL},
                         {stat, n_lanes * sizeof(vs_inverse_stat), VS_PART_DOWN, NULL}};
  rc = vs_host_begin(ctx, pcm, pcm_bytes, parts, 3);
  if (rc != VS_OK) return rc;
  rc = vs_inverse_launch(ctx, mode, order, (const int16_t *)ctx->pool.d_in, n_samples, (int16_t *)parts[0].dev, n_samples,
                         n_lanes, n_samples, rows, (const double *)parts[1].dev, sets_pitch,
                         (vs_inverse_stat *)parts[2].dev);
  return vs_host_end(ctx, rc, parts, 3);
}
