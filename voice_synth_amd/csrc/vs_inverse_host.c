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

static int check_call(int mode, int order, size_t in_pitch, size_t out_pitch, size_t n_lanes, size_t n_samples,
                      const vs_inverse_row *rows, size_t sets_pitch)
{
  if (n_lanes == 0 || n_samples == 0 || sets_pitch == 0 || in_pitch < n_samples || out_pitch < n_samples)
    return VS_ERR_ARG;
  if (mode != VS_TRACK_HOLD && mode != VS_TRACK_GLIDE) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || sets_pitch > 0x7FFFFFFFu || in_pitch > 0x7FFFFFFFu ||
      out_pitch > 0x7FFFFFFFu)
    return VS_ERR_UNSUPPORTED;
  if (order < 1 || order > VS_MAX_ORDER) return VS_ERR_RANGE;
  for (size_t i = 0; i < n_lanes; i++) {
    const vs_inverse_row *r = &rows[i];
    if (r->n_sets < 1 || (size_t)r->n_sets > sets_pitch || r->hop < 1 || r->length < 0 || (size_t)r->length > n_samples)
      return VS_ERR_RANGE;
    /* (written so that a NaN fails) */
    if (!(r->de_emphasis >= 0.0f && r->de_emphasis <= 1.0f) || !isfinite(r->scale)) return VS_ERR_RANGE;
  }
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
  /* 16-byte vector loads and stores need every row start 4-byte aligned */
  a.vec_ok = ((out_pitch & 1) == 0) && ((((uintptr_t)out_dev) & 3) == 0) && ((in_pitch & 1) == 0) &&
             ((((uintptr_t)pcm_dev) & 3) == 0);
  return vs_rec_retire(ctx, &blk, vs_launch_inverse(ctx->arith, mode, &a, ctx->stream));
}

int vs_inverse(vs_ctx *ctx, int mode, int order, const int16_t *pcm, int16_t *flow, size_t n_lanes, size_t n_samples,
               const vs_inverse_row *rows, const double *coefs, size_t sets_pitch, vs_inverse_stat *stat)
{
  if (!ctx || !pcm || !flow || !rows || !coefs) return VS_ERR_ARG;
  int rc = check_call(mode, order, n_samples, n_samples, n_lanes, n_samples, rows, sets_pitch);
  if (rc != VS_OK) return rc;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  /* the pool's buffers of the host-buffer paths (every such call waits before it returns, so they are idle here):
   * the speech in d_in; the flow, the sets and the status records in d_aux */
  const size_t pcm_bytes = n_lanes * n_samples * sizeof(int16_t), pcm_room = (pcm_bytes + 255) & ~(size_t)255;
  const size_t cf_bytes = n_lanes * sets_pitch * (size_t)(order + 1) * sizeof(double), cf_room = (cf_bytes + 255) & ~(size_t)255;
  const size_t st_bytes = stat ? n_lanes * sizeof(vs_inverse_stat) : 0;
  rc = vs_pool_device(ctx, &ctx->pool.d_in, &ctx->pool.d_in_bytes, pcm_bytes);
  if (rc == VS_OK) rc = vs_pool_device(ctx, &ctx->pool.d_aux, &ctx->pool.d_aux_bytes, pcm_room + cf_room + st_bytes);
  if (rc != VS_OK) return rc;
  char *aux = (char *)ctx->pool.d_aux;
  int16_t *d_flow = (int16_t *)aux;
  double *d_cf = (double *)(aux + pcm_room);
  vs_inverse_stat *d_st = stat ? (vs_inverse_stat *)(aux + pcm_room + cf_room) : NULL;
  VS_HIP(ctx, hipMemcpyAsync(ctx->pool.d_in, pcm, pcm_bytes, hipMemcpyHostToDevice, ctx->stream));
  /* what lies past a row's length comes back as it went */
  VS_HIP(ctx, hipMemcpyAsync(d_flow, flow, pcm_bytes, hipMemcpyHostToDevice, ctx->stream));
  VS_HIP(ctx, hipMemcpyAsync(d_cf, coefs, cf_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = vs_inverse_launch(ctx, mode, order, (const int16_t *)ctx->pool.d_in, n_samples, d_flow, n_samples, n_lanes,
                         n_samples, rows, d_cf, sets_pitch, d_st);
  if (rc != VS_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  VS_HIP(ctx, hipMemcpyAsync(flow, d_flow, pcm_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (d_st) VS_HIP(ctx, hipMemcpyAsync(stat, d_st, st_bytes, hipMemcpyDeviceToHost, ctx->stream));
  VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VS_OK;
}
