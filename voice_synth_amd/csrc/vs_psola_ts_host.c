/*
 * vs_psola_ts_host.c -- host side of PSOLA with a time map (include/voice_synth.h, "PSOLA with a time map"): the
 * options, the refusals of the sizes and strides, the row records, the scratch between the two kernels of
 * vs_psola_ts.hip, the launch and the host-buffer call.  Plain C against the HIP runtime's C API, like the rest of the
 * library's host side.  vs_psola_ts_check, vs_psola_ts_overlap, vs_psola_ts_fill and vs_psola_ts_scratch_bytes touch no
 * device (vs_psola_ts.h).
 */
#include <string.h>

#include "vs_psola_ts.h"
#include "vs_internal.h"

int vs_psola_ts_defaults(vs_psola_ts_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->pmin = 32;            /* vs_psola_defaults */
  opts->pmax = 320;
  opts->unvoiced_period = 80; /* 5 ms at 16 kHz */
  return VS_OK;
}

static int bad_stride(size_t s) { return s < 4 || (s & 3) != 0; }

int vs_psola_ts_check(const vs_psola_ts_opts *opts, size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch,
                      int has_segs, size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain,
                      size_t gain_stride, size_t count_stride, size_t target_pitch, size_t map_pitch, size_t out_pitch,
                      size_t out_samples, size_t synth_pitch, vs_psola_ts_opts *resolved)
{
  if (n_lanes == 0 || n_samples == 0 || out_samples == 0 || marks_pitch == 0 || target_pitch == 0) return VS_ERR_ARG;
  if (pitch < n_samples || out_pitch < out_samples || synth_pitch < 2 || map_pitch < 2) return VS_ERR_ARG;
  if (has_segs && seg_pitch == 0) return VS_ERR_ARG;
  if (bad_stride(start_stride) || bad_stride(period_stride) || bad_stride(count_stride)) return VS_ERR_ARG;
  if (has_gain && bad_stride(gain_stride)) return VS_ERR_ARG;
  if (opts) *resolved = *opts;
  else vs_psola_ts_defaults(resolved);
  if (resolved->reserved_ != 0) return VS_ERR_ARG;
  const size_t lim = 0x7FFFFFFFu;
  if (pitch > lim || n_lanes > lim || n_samples > lim || marks_pitch > lim || seg_pitch > lim || start_stride > lim ||
      period_stride > lim || gain_stride > lim || count_stride > lim || target_pitch > lim || map_pitch > lim ||
      out_pitch > lim || out_samples > lim || synth_pitch > lim)
    return VS_ERR_UNSUPPORTED;
  if (vs_psola_tiles(out_samples) > lim / n_lanes) return VS_ERR_UNSUPPORTED; /* one workgroup per (row, output tile) */
  if (resolved->pmin < 2 || resolved->pmax > VS_AC_MAX_LAG || resolved->pmin > resolved->pmax) return VS_ERR_RANGE;
  if (resolved->unvoiced_period < 2 || resolved->unvoiced_period > 2 * VS_AC_MAX_LAG / 3) return VS_ERR_RANGE;
  return VS_OK;
}

/* the bytes from the first row's first sample to the last row's last, of both batches */
int vs_psola_ts_overlap(const void *a, size_t a_pitch, size_t a_samples, const void *b, size_t b_pitch, size_t b_samples,
                        size_t n_lanes)
{
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  const uintptr_t a1 = a0 + ((n_lanes - 1) * a_pitch + a_samples) * sizeof(int16_t);
  const uintptr_t b1 = b0 + ((n_lanes - 1) * b_pitch + b_samples) * sizeof(int16_t);
  return a0 < b1 && b0 < a1;
}

int vs_psola_ts_fill(const int32_t *lengths, const int32_t *out_lengths, size_t n_lanes, size_t n_samples,
                     size_t out_samples, VsPtRow *rows)
{
  for (size_t i = 0; i < n_lanes; i++) {
    const int32_t len = lengths ? lengths[i] : (int32_t)n_samples;
    const int32_t len_out = out_lengths ? out_lengths[i] : (int32_t)out_samples;
    if (len < 0 || (size_t)len > n_samples || len_out < 0 || (size_t)len_out > out_samples) return VS_ERR_RANGE;
    if (rows) {
      rows[i].length = len;
      rows[i].len_out = len_out;
    }
  }
  return VS_OK;
}

size_t vs_psola_ts_scratch_bytes(size_t n_lanes, size_t synth_pitch) { return n_lanes * synth_pitch * sizeof(VsPtAux); }

int vs_psola_ts_launch(vs_ctx *ctx, const vs_psola_ts_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                       size_t n_samples, const int32_t *lengths, const int32_t *marks_dev, size_t marks_pitch,
                       const vs_guided_rec *rec_dev, const vs_guided_seg *segs_dev, size_t seg_pitch,
                       const int32_t *start_dev, size_t start_stride, const int32_t *period_dev, size_t period_stride,
                       const int32_t *gain_dev, size_t gain_stride, const int32_t *count_dev, size_t count_stride,
                       size_t target_pitch, const vs_psola_anchor *map_dev, const int32_t *map_count_dev,
                       size_t map_pitch, int16_t *out_dev, size_t out_pitch, size_t out_samples,
                       const int32_t *out_lengths, vs_psola_stat *stat_dev, vs_psola_mark *synth_dev, size_t synth_pitch)
{
  vs_psola_ts_opts o;
  if (!ctx || !pcm_dev || !marks_dev || !rec_dev || !start_dev || !period_dev || !count_dev || !map_dev ||
      !map_count_dev || !out_dev || !stat_dev || !synth_dev)
    return VS_ERR_ARG;
  if (((uintptr_t)pcm_dev & 1) != 0 || ((uintptr_t)out_dev & 1) != 0) return VS_ERR_ARG;
  if ((((uintptr_t)marks_dev | (uintptr_t)rec_dev | (uintptr_t)segs_dev | (uintptr_t)start_dev | (uintptr_t)period_dev |
        (uintptr_t)gain_dev | (uintptr_t)count_dev | (uintptr_t)map_dev | (uintptr_t)map_count_dev |
        (uintptr_t)stat_dev | (uintptr_t)synth_dev) & 3) != 0)
    return VS_ERR_ARG;
  int rc = vs_psola_ts_check(opts, pitch, n_lanes, n_samples, marks_pitch, segs_dev != NULL, seg_pitch, start_stride,
                             period_stride, gain_dev != NULL, gain_stride, count_stride, target_pitch, map_pitch,
                             out_pitch, out_samples, synth_pitch, &o);
  if (rc == VS_ERR_ARG) return rc;
  /* (sizes beyond 2^31 are refused before the products below are formed with them) */
  if (rc != VS_ERR_UNSUPPORTED && vs_psola_ts_overlap(pcm_dev, pitch, n_samples, out_dev, out_pitch, out_samples, n_lanes))
    return VS_ERR_ARG;
  if (rc != VS_OK) return rc;

  const size_t bytes = n_lanes * sizeof(VsPtRow);
  void *host = NULL;
  rc = vs_rec_stage(ctx, &ctx->rec_psola_ts, bytes, &host);
  if (rc != VS_OK) return rc;
  rc = vs_psola_ts_fill(lengths, out_lengths, n_lanes, n_samples, out_samples, (VsPtRow *)host);
  if (rc != VS_OK) return rc;

  /* the scratch between the kernels: a block of the same cache, retired behind the same kernels */
  VsRecBlock blk, scratch;
  scratch.dev = NULL;
  scratch.cap = 0;
  hipError_t e = plan_block_get(ctx, vs_psola_ts_scratch_bytes(n_lanes, synth_pitch), &scratch.dev, &scratch.cap);
  if (e != hipSuccess) {
    ctx->last_hip_error = (int)e;
    return VS_ERR_HIP;
  }
  rc = vs_rec_upload(ctx, &ctx->rec_psola_ts, bytes, &blk);
  if (rc != VS_OK) {
    plan_block_put(ctx, scratch.dev, scratch.cap, NULL); /* nothing was enqueued that reads it */
    return rc;
  }
  VsPtArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm_dev;
  a.pitch = (long)pitch;
  a.n_lanes = (long)n_lanes;
  a.out_samples = (long)out_samples;
  a.rows = (const VsPtRow *)blk.dev;
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
  a.map = map_dev;
  a.map_count = map_count_dev;
  a.map_pitch = (long)map_pitch;
  a.out = out_dev;
  a.out_pitch = (long)out_pitch;
  a.stat = stat_dev;
  a.synth = synth_dev;
  a.aux = (VsPtAux *)scratch.dev;
  a.synth_pitch = (long)synth_pitch;
  a.pmin = o.pmin;
  a.pmax = o.pmax;
  a.unvoiced = o.unvoiced_period;
  const hipError_t launched = vs_launch_psola_ts(&a, ctx->stream);
  rc = vs_rec_retire(ctx, &blk, launched);
  const int rc2 = vs_rec_retire(ctx, &scratch, launched);
  return rc != VS_OK ? rc : rc2;
}

int vs_psola_ts(vs_ctx *ctx, const vs_psola_ts_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes,
                size_t n_samples, const int32_t *lengths, const int32_t *marks, size_t marks_pitch,
                const vs_guided_rec *rec, const vs_guided_seg *segs, size_t seg_pitch, const int32_t *start,
                const int32_t *period, const int32_t *gain, const int32_t *count, size_t target_pitch,
                const vs_psola_anchor *map, const int32_t *map_count, size_t map_pitch, int16_t *out, size_t out_samples,
                const int32_t *out_lengths, vs_psola_stat *stat, vs_psola_mark *synth, size_t synth_pitch)
{
  vs_psola_ts_opts o;
  if (!ctx || !pcm || !marks || !rec || !start || !period || !count || !map || !map_count || !out || !stat || !synth)
    return VS_ERR_ARG;
  int rc = vs_psola_ts_check(opts, pitch, n_lanes, n_samples, marks_pitch, segs != NULL, seg_pitch, 4, 4, gain != NULL, 4,
                             4, target_pitch, map_pitch, out_samples, out_samples, synth_pitch, &o);
  if (rc != VS_OK) return rc;
  rc = vs_psola_ts_fill(lengths, out_lengths, n_lanes, n_samples, out_samples, NULL); /* refused before anything moves */
  if (rc != VS_OK) return rc;
  /* the PCM in d_in; the marks, the runs, the target and the map go up; the output and the synthesis marks go up and come
   * back (what lies past a row's output length or its marks comes back as it went); the status records come back */
  const size_t tb = n_lanes * target_pitch * sizeof(int32_t);
  VsHostPart parts[12] = {{(void *)marks, n_lanes * marks_pitch * sizeof(int32_t), VS_PART_UP, NULL},
                          {(void *)rec, n_lanes * sizeof(vs_guided_rec), VS_PART_UP, NULL},
                          {(void *)segs, n_lanes * seg_pitch * sizeof(vs_guided_seg), VS_PART_UP, NULL},
                          {(void *)start, tb, VS_PART_UP, NULL},
                          {(void *)period, tb, VS_PART_UP, NULL},
                          {(void *)gain, tb, VS_PART_UP, NULL},
                          {(void *)count, n_lanes * sizeof(int32_t), VS_PART_UP, NULL},
                          {(void *)map, n_lanes * map_pitch * sizeof(vs_psola_anchor), VS_PART_UP, NULL},
                          {(void *)map_count, n_lanes * sizeof(int32_t), VS_PART_UP, NULL},
                          {out, n_lanes * out_samples * sizeof(int16_t), VS_PART_UP | VS_PART_DOWN, NULL},
                          {stat, n_lanes * sizeof(vs_psola_stat), VS_PART_DOWN, NULL},
                          {synth, n_lanes * synth_pitch * sizeof(vs_psola_mark), VS_PART_UP | VS_PART_DOWN, NULL}};
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 12);
  if (rc != VS_OK) return rc;
  rc = vs_psola_ts_launch(ctx, &o, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, lengths,
                          (const int32_t *)parts[0].dev, marks_pitch, (const vs_guided_rec *)parts[1].dev,
                          (const vs_guided_seg *)parts[2].dev, seg_pitch, (const int32_t *)parts[3].dev, 4,
                          (const int32_t *)parts[4].dev, 4, (const int32_t *)parts[5].dev, 4, (const int32_t *)parts[6].dev, 4,
                          target_pitch, (const vs_psola_anchor *)parts[7].dev, (const int32_t *)parts[8].dev, map_pitch,
                          (int16_t *)parts[9].dev, out_samples, out_samples, out_lengths, (vs_psola_stat *)parts[10].dev,
                          (vs_psola_mark *)parts[11].dev, synth_pitch);
  return vs_host_end(ctx, rc, parts, 12);
}
