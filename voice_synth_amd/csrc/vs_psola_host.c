/*
 * vs_psola_host.c -- host side of PSOLA (include/voice_synth.h, "PSOLA"): the options, the refusals of the sizes and
 * strides, the row records, the scratch between the two kernels of vs_psola.hip, the launch and the host-buffer call.
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.  vs_psola_check, vs_psola_fill,
 * vs_psola_tiles and vs_psola_scratch_bytes touch no device (vs_psola.h).
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

int vs_psola_check(const vs_psola_opts *opts, size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch,
                   int has_segs, size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain,
                   size_t gain_stride, size_t count_stride, size_t target_pitch, size_t out_pitch, size_t synth_pitch,
                   vs_psola_opts *resolved)
{
  if (n_lanes == 0 || n_samples == 0 || marks_pitch == 0 || target_pitch == 0) return VS_ERR_ARG;
  if (pitch < n_samples || out_pitch < n_samples || synth_pitch < 2) return VS_ERR_ARG;
  if (has_segs && seg_pitch == 0) return VS_ERR_ARG;
  if (bad_stride(start_stride) || bad_stride(period_stride) || bad_stride(count_stride)) return VS_ERR_ARG;
  if (has_gain && bad_stride(gain_stride)) return VS_ERR_ARG;
  if (opts) *resolved = *opts;
  else vs_psola_defaults(resolved);
  if (resolved->reserved_[0] != 0 || resolved->reserved_[1] != 0) return VS_ERR_ARG;
  const size_t lim = 0x7FFFFFFFu;
  if (pitch > lim || n_lanes > lim || n_samples > lim || marks_pitch > lim || seg_pitch > lim || start_stride > lim ||
      period_stride > lim || gain_stride > lim || count_stride > lim || target_pitch > lim || out_pitch > lim ||
      synth_pitch > lim)
    return VS_ERR_UNSUPPORTED;
  if (vs_psola_tiles(n_samples) > lim / n_lanes) return VS_ERR_UNSUPPORTED; /* one workgroup per (row, tile) */
  if (resolved->pmin < 2 || resolved->pmax > VS_AC_MAX_LAG || resolved->pmin > resolved->pmax) return VS_ERR_RANGE;
  return VS_OK;
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
  if (!ctx || !pcm_dev || !marks_dev || !rec_dev || !start_dev || !period_dev || !count_dev || !out_dev || !stat_dev ||
      !synth_dev)
    return VS_ERR_ARG;
  if (((uintptr_t)pcm_dev & 1) != 0 || ((uintptr_t)out_dev & 1) != 0) return VS_ERR_ARG;
  if ((((uintptr_t)marks_dev | (uintptr_t)rec_dev | (uintptr_t)segs_dev | (uintptr_t)start_dev | (uintptr_t)period_dev |
        (uintptr_t)gain_dev | (uintptr_t)count_dev | (uintptr_t)stat_dev | (uintptr_t)synth_dev) & 3) != 0)
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
  scratch.dev = NULL;
  scratch.cap = 0;
  hipError_t e = plan_block_get(ctx, vs_psola_scratch_bytes(n_lanes, synth_pitch), &scratch.dev, &scratch.cap);
  if (e != hipSuccess) {
    ctx->last_hip_error = (int)e;
    return VS_ERR_HIP;
  }
  rc = vs_rec_upload(ctx, &ctx->rec_psola, bytes, &blk);
  if (rc != VS_OK) {
    plan_block_put(ctx, scratch.dev, scratch.cap, NULL); /* nothing was enqueued that reads it */
    return rc;
  }
  VsPsArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm_dev;
  a.pitch = (long)pitch;
  a.n_lanes = (long)n_lanes;
  a.n_samples = (long)n_samples;
  a.rows = (const VsPsRow *)blk.dev;
  a.marks = marks_dev;
  a.marks_pitch = (long)marks_pitch;
  a.rec = rec_dev;
  a.segs = segs_dev;
  a.seg_pitch = segs_dev ? (long)seg_pitch : 0;
  a.start = (const char *)start_dev;
  a.period = (const char *)period_dev;
  a.gain = (const char *)gain_dev;
  a.count = (const char *)count_dev;
  a.start_stride = (int)start_stride;
  a.period_stride = (int)period_stride;
  a.gain_stride = gain_dev ? (int)gain_stride : 0;
  a.count_stride = (int)count_stride;
  a.target_pitch = (long)target_pitch;
  a.out = out_dev;
  a.out_pitch = (long)out_pitch;
  a.stat = stat_dev;
  a.synth = synth_dev;
  a.aux = (VsPsAux *)scratch.dev;
  a.synth_pitch = (long)synth_pitch;
  a.pmin = o.pmin;
  a.pmax = o.pmax;
  const hipError_t launched = vs_launch_psola(&a, ctx->stream);
  rc = vs_rec_retire(ctx, &blk, launched);
  const int rc2 = vs_rec_retire(ctx, &scratch, launched);
  return rc != VS_OK ? rc : rc2;
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
  const size_t tb = n_lanes * target_pitch * sizeof(int32_t);
  VsHostPart parts[10] = {{(void *)marks, n_lanes * marks_pitch * sizeof(int32_t), VS_PART_UP, NULL},
                          {(void *)rec, n_lanes * sizeof(vs_guided_rec), VS_PART_UP, NULL},
                          {(void *)segs, n_lanes * seg_pitch * sizeof(vs_guided_seg), VS_PART_UP, NULL},
                          {(void *)start, tb, VS_PART_UP, NULL},
                          {(void *)period, tb, VS_PART_UP, NULL},
                          {(void *)gain, tb, VS_PART_UP, NULL},
                          {(void *)count, n_lanes * sizeof(int32_t), VS_PART_UP, NULL},
                          {out, n_lanes * n_samples * sizeof(int16_t), VS_PART_UP | VS_PART_DOWN, NULL},
                          {stat, n_lanes * sizeof(vs_psola_stat), VS_PART_DOWN, NULL},
                          {synth, n_lanes * synth_pitch * sizeof(vs_psola_mark), VS_PART_UP | VS_PART_DOWN, NULL}};
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
