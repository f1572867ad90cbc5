/*
 * vs_psola_host.c -- host side of PSOLA (include/voice_synth.h, "PSOLA"): the options, the refusals of the sizes and
 * strides, the row records, the scratch between the two kernels of vs_psola.hip, the launch and the host-buffer call.
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.  vs_psola_check, vs_psola_fill,
 * vs_psola_tiles and vs_psola_scratch_bytes touch no device (vs_psola.h).  What PSOLA with a time map does alike lives
 * here too and vs_psola_ts_host.c calls it: vs_psola_common_check, vs_psola_bad_pointers, vs_psola_common, vs_psola_parts.
 */
#include <string.h>

#include "vs_psola.h"
#include "vs_internal.h"

int vs_psola_defaults(vs_psola_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->pmin = 32;  /* floor(16000 / 500) */
  opts->pmax = 320; /* ceil(16000 / 50) */
  return VS_OK;
}

static int bad_stride(size_t s) { return s < 4 || (s & 3) != 0; }

/* What vs_psola_check and vs_psola_ts_check refuse alike, the first of VS_ERR_ARG, VS_ERR_UNSUPPORTED, VS_ERR_RANGE.
 * out_samples: the output row's samples (PSOLA: n_samples); pmin, pmax: the resolved options. */
int vs_psola_common_check(size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch, int has_segs,
                          size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain, size_t gain_stride,
                          size_t count_stride, size_t target_pitch, size_t out_pitch, size_t out_samples,
                          size_t synth_pitch, int pmin, int pmax)
{
  if (n_lanes == 0 || n_samples == 0 || out_samples == 0 || marks_pitch == 0 || target_pitch == 0) return VS_ERR_ARG;
  if (pitch < n_samples || out_pitch < out_samples || synth_pitch < 2) return VS_ERR_ARG;
  if (has_segs && seg_pitch == 0) return VS_ERR_ARG;
  if (bad_stride(start_stride) || bad_stride(period_stride) || bad_stride(count_stride)) return VS_ERR_ARG;
  if (has_gain && bad_stride(gain_stride)) return VS_ERR_ARG;
  const size_t lim = 0x7FFFFFFFu;
  if (pitch > lim || n_lanes > lim || n_samples > lim || marks_pitch > lim || seg_pitch > lim || start_stride > lim ||
      period_stride > lim || gain_stride > lim || count_stride > lim || target_pitch > lim || out_pitch > lim ||
      out_samples > lim || synth_pitch > lim)
    return VS_ERR_UNSUPPORTED;
  if (vs_psola_tiles(out_samples) > lim / n_lanes) return VS_ERR_UNSUPPORTED; /* one workgroup per (row, output tile) */
  if (pmin < 2 || pmax > VS_AC_MAX_LAG || pmin > pmax) return VS_ERR_RANGE;
  return VS_OK;
}

int vs_psola_check(const vs_psola_opts *opts, size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch,
                   int has_segs, size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain,
                   size_t gain_stride, size_t count_stride, size_t target_pitch, size_t out_pitch, size_t synth_pitch,
                   vs_psola_opts *resolved)
{
  vs_psola_opts o;
  if (opts) o = *opts;
  else vs_psola_defaults(&o);
  const int rc = vs_psola_common_check(pitch, n_lanes, n_samples, marks_pitch, has_segs, seg_pitch, start_stride,
                                       period_stride, has_gain, gain_stride, count_stride, target_pitch, out_pitch,
                                       n_samples, synth_pitch, o.pmin, o.pmax);
  if (rc == VS_ERR_ARG) return rc; /* (*resolved is written only behind the refusals of the sizes and strides) */
  *resolved = o;
  if (o.reserved_[0] != 0 || o.reserved_[1] != 0) return VS_ERR_ARG;
  return rc;
}

/* a pointer either launch needs is missing, or one is not aligned to its element (segs and gain may be NULL) */
int vs_psola_bad_pointers(const vs_ctx *ctx, const int16_t *pcm_dev, const int32_t *marks_dev,
                          const vs_guided_rec *rec_dev, const vs_guided_seg *segs_dev, const int32_t *start_dev,
                          const int32_t *period_dev, const int32_t *gain_dev, const int32_t *count_dev,
                          const int16_t *out_dev, const vs_psola_stat *stat_dev, const vs_psola_mark *synth_dev)
{
  if (!ctx || !pcm_dev || !marks_dev || !rec_dev || !start_dev || !period_dev || !count_dev || !out_dev || !stat_dev ||
      !synth_dev)
    return 1;
  if (((uintptr_t)pcm_dev & 1) != 0 || ((uintptr_t)out_dev & 1) != 0) return 1;
  return (((uintptr_t)marks_dev | (uintptr_t)rec_dev | (uintptr_t)segs_dev | (uintptr_t)start_dev |
           (uintptr_t)period_dev | (uintptr_t)gain_dev | (uintptr_t)count_dev | (uintptr_t)stat_dev |
           (uintptr_t)synth_dev) & 3) != 0;
}

void vs_psola_common(VsPsCommon *c, int pmin, int pmax, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                     const int32_t *marks_dev, size_t marks_pitch, const vs_guided_rec *rec_dev,
                     const vs_guided_seg *segs_dev, size_t seg_pitch, const int32_t *start_dev, size_t start_stride,
                     const int32_t *period_dev, size_t period_stride, const int32_t *gain_dev, size_t gain_stride,
                     const int32_t *count_dev, size_t count_stride, size_t target_pitch, int16_t *out_dev,
                     size_t out_pitch, vs_psola_stat *stat_dev, vs_psola_mark *synth_dev, size_t synth_pitch)
{
  c->pcm = pcm_dev;
  c->pitch = (long)pitch;
  c->n_lanes = (long)n_lanes;
  c->marks = marks_dev;
  c->marks_pitch = (long)marks_pitch;
  c->rec = rec_dev;
  c->segs = segs_dev;
  c->seg_pitch = segs_dev ? (long)seg_pitch : 0;
  c->start = (const char *)start_dev;
  c->period = (const char *)period_dev;
  c->gain = (const char *)gain_dev;
  c->count = (const char *)count_dev;
  c->start_stride = (int)start_stride;
  c->period_stride = (int)period_stride;
  c->gain_stride = gain_dev ? (int)gain_stride : 0;
  c->count_stride = (int)count_stride;
  c->target_pitch = (long)target_pitch;
  c->out = out_dev;
  c->out_pitch = (long)out_pitch;
  c->stat = stat_dev;
  c->synth = synth_dev;
  c->synth_pitch = (long)synth_pitch;
  c->pmin = pmin;
  c->pmax = pmax;
}

/* the first seven parts of either host-buffer call: the marks, the runs and the target go up */
void vs_psola_parts(VsHostPart *parts, size_t n_lanes, const int32_t *marks, size_t marks_pitch, const vs_guided_rec *rec,
                    const vs_guided_seg *segs, size_t seg_pitch, const int32_t *start, const int32_t *period,
                    const int32_t *gain, const int32_t *count, size_t target_pitch)
{
  const size_t tb = n_lanes * target_pitch * sizeof(int32_t);
  const VsHostPart up[7] = {{(void *)marks, n_lanes * marks_pitch * sizeof(int32_t), VS_PART_UP, NULL},
                            {(void *)rec, n_lanes * sizeof(vs_guided_rec), VS_PART_UP, NULL},
                            {(void *)segs, n_lanes * seg_pitch * sizeof(vs_guided_seg), VS_PART_UP, NULL},
                            {(void *)start, tb, VS_PART_UP, NULL},
                            {(void *)period, tb, VS_PART_UP, NULL},
                            {(void *)gain, tb, VS_PART_UP, NULL},
                            {(void *)count, n_lanes * sizeof(int32_t), VS_PART_UP, NULL}};
  memcpy(parts, up, sizeof(up));
}

int vs_psola_fill(const int32_t *lengths, size_t n_lanes, size_t n_samples, VsPsRow *rows)
{
  for (size_t i = 0; i < n_lanes; i++) {
    const int32_t len = lengths ? lengths[i] : (int32_t)n_samples;
    if (len < 0 || (size_t)len > n_samples) return VS_ERR_RANGE;
    rows[i].length = len;
  }
  return VS_OK;
}

/* a row's first sample lies up to VS_PS_PER_LANE - 1 samples behind a 16-byte address */
size_t vs_psola_tiles(size_t n_samples) { return (n_samples + (VS_PS_PER_LANE - 1) + (VS_PS_TILE - 1)) / VS_PS_TILE; }

size_t vs_psola_scratch_bytes(size_t n_lanes, size_t synth_pitch) { return n_lanes * synth_pitch * sizeof(VsPsAux); }

int vs_psola_launch(vs_ctx *ctx, const vs_psola_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                    size_t n_samples, const int32_t *lengths, const int32_t *marks_dev, size_t marks_pitch,
                    const vs_guided_rec *rec_dev, const vs_guided_seg *segs_dev, size_t seg_pitch,
                    const int32_t *start_dev, size_t start_stride, const int32_t *period_dev, size_t period_stride,
                    const int32_t *gain_dev, size_t gain_stride, const int32_t *count_dev, size_t count_stride,
                    size_t target_pitch, int16_t *out_dev, size_t out_pitch, vs_psola_stat *stat_dev,
                    vs_psola_mark *synth_dev, size_t synth_pitch)
{
  vs_psola_opts o;
  if (vs_psola_bad_pointers(ctx, pcm_dev, marks_dev, rec_dev, segs_dev, start_dev, period_dev, gain_dev, count_dev, out_dev,
                            stat_dev, synth_dev))
    return VS_ERR_ARG;
  int rc = vs_psola_check(opts, pitch, n_lanes, n_samples, marks_pitch, segs_dev != NULL, seg_pitch, start_stride,
                          period_stride, gain_dev != NULL, gain_stride, count_stride, target_pitch, out_pitch,
                          synth_pitch, &o);
  if (rc != VS_OK) return rc;

  const size_t bytes = n_lanes * sizeof(VsPsRow);
  void *host = NULL;
  rc = vs_rec_stage(ctx, &ctx->rec_psola, bytes, &host);
  if (rc != VS_OK) return rc;
  rc = vs_psola_fill(lengths, n_lanes, n_samples, (VsPsRow *)host);
  if (rc != VS_OK) return rc;

  /* the scratch between the kernels: a block of the same cache, retired behind the same kernels */
  VsRecBlock blk, scratch;
  rc = vs_rec_upload_scratch(ctx, &ctx->rec_psola, bytes, &blk, vs_psola_scratch_bytes(n_lanes, synth_pitch), &scratch);
  if (rc != VS_OK) return rc;
  VsPsArgs a;
  memset(&a, 0, sizeof(a));
  vs_psola_common(&a.c, o.pmin, o.pmax, pcm_dev, pitch, n_lanes, marks_dev, marks_pitch, rec_dev, segs_dev, seg_pitch,
                  start_dev, start_stride, period_dev, period_stride, gain_dev, gain_stride, count_dev, count_stride,
                  target_pitch, out_dev, out_pitch, stat_dev, synth_dev, synth_pitch);
  a.n_samples = (long)n_samples;
  a.rows = (const VsPsRow *)blk.dev;
  a.aux = (VsPsAux *)scratch.dev;
  return vs_rec_retire_both(ctx, &blk, &scratch, vs_launch_psola(&a, ctx->stream));
}

int vs_psola(vs_ctx *ctx, const vs_psola_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
             const int32_t *lengths, const int32_t *marks, size_t marks_pitch, const vs_guided_rec *rec,
             const vs_guided_seg *segs, size_t seg_pitch, const int32_t *start, const int32_t *period,
             const int32_t *gain, const int32_t *count, size_t target_pitch, int16_t *out, vs_psola_stat *stat,
             vs_psola_mark *synth, size_t synth_pitch)
{
  vs_psola_opts o;
  if (!ctx || !pcm || !marks || !rec || !start || !period || !count || !out || !stat || !synth) return VS_ERR_ARG;
  int rc = vs_psola_check(opts, pitch, n_lanes, n_samples, marks_pitch, segs != NULL, seg_pitch, 4, 4, gain != NULL, 4, 4,
                          target_pitch, n_samples, synth_pitch, &o);
  if (rc != VS_OK) return rc;
  if (lengths) /* refused before anything moves */
    for (size_t i = 0; i < n_lanes; i++)
      if (lengths[i] < 0 || (size_t)lengths[i] > n_samples) return VS_ERR_RANGE;
  /* the PCM in d_in; the marks, the runs and the target go up; the output and the synthesis marks go up and come back
   * (what lies past a row's length or its marks comes back as it went); the status records come back */
  VsHostPart parts[10] = {[7] = {out, n_lanes * n_samples * sizeof(int16_t), VS_PART_UP | VS_PART_DOWN, NULL},
                          {stat, n_lanes * sizeof(vs_psola_stat), VS_PART_DOWN, NULL},
                          {synth, n_lanes * synth_pitch * sizeof(vs_psola_mark), VS_PART_UP | VS_PART_DOWN, NULL}};
  vs_psola_parts(parts, n_lanes, marks, marks_pitch, rec, segs, seg_pitch, start, period, gain, count, target_pitch);
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 10);
  if (rc != VS_OK) return rc;
  rc = vs_psola_launch(ctx, &o, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, lengths,
                       (const int32_t *)parts[0].dev, marks_pitch, (const vs_guided_rec *)parts[1].dev,
                       (const vs_guided_seg *)parts[2].dev, seg_pitch, (const int32_t *)parts[3].dev, 4,
                       (const int32_t *)parts[4].dev, 4, (const int32_t *)parts[5].dev, 4, (const int32_t *)parts[6].dev, 4,
                       target_pitch, (int16_t *)parts[7].dev, n_samples, (vs_psola_stat *)parts[8].dev,
                       (vs_psola_mark *)parts[9].dev, synth_pitch);
  return vs_host_end(ctx, rc, parts, 10);
}
