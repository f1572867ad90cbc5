/*
 * vs_acoustic_host.c -- host side of the acoustic measurement (include/voice_synth.h, "acoustic measurement"):
 * the options, the lag bounds of every row, the upload of the per-row records, the two kernels of vs_acoustic.hip.
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.
 */
#include <math.h>
#include <string.h>

#include "vs_acoustic.h"
#include "vs_internal.h"

int vs_measure_defaults(vs_measure_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  opts->f0_min = 50.0f; /* fg:504 */
  opts->f0_max = 500.0f;
  opts->polarity = 1;
  opts->reserved_ = 0;
  return VS_OK;
}

/* lag bounds of one row (the header's formulas, in double); VS_ERR_RANGE outside the limits */
static int lag_bounds(int32_t fs, const vs_measure_opts *o, int32_t *tmin, int32_t *tmax)
{
  if (fs <= 0) return VS_ERR_RANGE;
  const double lo = floor((double)fs / (double)o->f0_max), hi = ceil((double)fs / (double)o->f0_min);
  if (!(lo >= 2.0) || !(hi <= (double)VS_AC_MAX_LAG) || !(lo < hi)) return VS_ERR_RANGE;
  *tmin = (int32_t)lo;
  *tmax = (int32_t)hi;
  return VS_OK;
}

static int check_opts(const vs_measure_opts *o)
{
  if (!(o->f0_min > 0.0f) || !(o->f0_max > 0.0f) || !isfinite(o->f0_min) || !isfinite(o->f0_max)) return VS_ERR_ARG;
  if ((o->polarity != 1 && o->polarity != -1) || o->reserved_ != 0) return VS_ERR_ARG;
  return VS_OK;
}

int vs_measure_launch(vs_ctx *ctx, const vs_measure_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                      size_t n_samples, const int32_t *fs, const int32_t *lengths, vs_acoustic *out_dev,
                      int32_t *marks_dev, size_t marks_pitch)
{
  vs_measure_opts o;
  if (!ctx || !pcm_dev || !fs || !out_dev || n_lanes == 0 || n_samples == 0 || pitch < n_samples) return VS_ERR_ARG;
  if (marks_dev && marks_pitch == 0) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || marks_pitch > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED;
  if (opts) o = *opts;
  else vs_measure_defaults(&o);
  int rc = check_opts(&o);
  if (rc != VS_OK) return rc;

  const size_t bytes = n_lanes * sizeof(VsAcRow);
  void *host = NULL;
  rc = vs_rec_stage(ctx, &ctx->rec_measure, bytes, &host);
  if (rc != VS_OK) return rc;
  VsAcRow *rows = (VsAcRow *)host;
  int lds = 0;
  for (size_t i = 0; i < n_lanes; i++) {
    VsAcRow *r = &rows[i];
    const int32_t len = lengths ? lengths[i] : (int32_t)n_samples;
    if (len < 0 || (size_t)len > n_samples) return VS_ERR_ARG;
    rc = lag_bounds(fs[i], &o, &r->tmin, &r->tmax);
    if (rc != VS_OK) return rc;
    r->len = len;
    r->fs = fs[i];
    const int l = vs_ac_lds_doubles(r->tmin, r->tmax);
    if (l > lds) lds = l;
  }

  VsRecBlock blk;
  rc = vs_rec_upload(ctx, &ctx->rec_measure, bytes, &blk);
  if (rc != VS_OK) return rc;
  VsAcArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm_dev;
  a.pitch = (long)pitch;
  a.n_lanes = (long)n_lanes;
  a.n_samples = (long)n_samples;
  a.rows = (const VsAcRow *)blk.dev;
  a.out = out_dev;
  a.marks = marks_dev;
  a.marks_pitch = marks_dev ? (long)marks_pitch : 0;
  a.polarity = o.polarity;
  return vs_rec_retire(ctx, &blk, vs_launch_measure(&a, lds, ctx->stream));
}

int vs_measure(vs_ctx *ctx, const vs_measure_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes,
               size_t n_samples, const int32_t *fs, const int32_t *lengths, vs_acoustic *out, int32_t *marks,
               size_t marks_pitch)
{
  if (!ctx || !pcm || !fs || !out || n_lanes == 0 || n_samples == 0 || pitch < n_samples) return VS_ERR_ARG;
  if (marks && marks_pitch == 0) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || marks_pitch > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED;
  /* the PCM in d_in; the records come back, the marks are filled with -1 (past the last mark) and come back */
  VsHostPart parts[2] = {{out, n_lanes * sizeof(vs_acoustic), VS_PART_DOWN, NULL},
                         {marks, n_lanes * marks_pitch * sizeof(int32_t), VS_PART_FILL_FF | VS_PART_DOWN, NULL}};
  int rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 2);
  if (rc != VS_OK) return rc;
  rc = vs_measure_launch(ctx, opts, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths,
                         (vs_acoustic *)parts[0].dev, (int32_t *)parts[1].dev, marks_pitch);
  return vs_host_end(ctx, rc, parts, 2);
}
