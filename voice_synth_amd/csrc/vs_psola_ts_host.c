/*
 * vs_psola_ts_host.c -- host side of PSOLA with a time map (include/voice_synth.h, "PSOLA with a time map"): the
 * options, the refusals of the sizes and strides, the row records, the scratch between the two kernels of
 * vs_psola_ts.hip, the launch and the host-buffer call.  Plain C against the HIP runtime's C API, like the rest of the
 * library's host side.  vs_psola_ts_check, vs_psola_ts_overlap, vs_psola_ts_fill and vs_psola_ts_scratch_bytes touch no
 * device (vs_psola_ts.h).  The refusals, pointer checks, launch arguments and host parts it has in common with PSOLA
 * are vs_psola_host.c's.
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

int vs_psola_ts_check(const vs_psola_ts_opts *opts, size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch,
                      int has_segs, size_t seg_pitch, size_t start_stride, size_t period_stride, int has_gain,
                      size_t gain_stride, size_t count_stride, size_t target_pitch, size_t map_pitch, size_t out_pitch,
                      size_t out_samples, size_t synth_pitch, vs_psola_ts_opts *resolved)
{
  vs_psola_ts_opts o;
  if (opts) o = *opts;
  else vs_psola_ts_defaults(&o);
  const int rc = vs_psola_common_check(pitch, n_lanes, n_samples, marks_pitch, has_segs, seg_pitch, start_stride,
                                       period_stride, has_gain, gain_stride, count_stride, target_pitch, out_pitch,
                                       out_samples, synth_pitch, o.pmin, o.pmax);
  if (rc == VS_ERR_ARG || map_pitch < 2) return VS_ERR_ARG; /* (*resolved is written only behind these) */
  *resolved = o;
  if (o.reserved_ != 0) return VS_ERR_ARG;
  if (rc == VS_ERR_UNSUPPORTED || map_pitch > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED;
  if (rc != VS_OK) return rc;
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
  if (vs_psola_bad_pointers(ctx, pcm_dev, marks_dev, rec_dev, segs_dev, start_dev, period_dev, gain_dev, count_dev, out_dev,
                            stat_dev, synth_dev))
    return VS_ERR_ARG;
  if (!map_dev || !map_count_dev || (((uintptr_t)map_dev | (uintptr_t)map_count_dev) & 3) != 0) return VS_ERR_ARG;
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
  rc = vs_rec_upload_scratch(ctx, &ctx->rec_psola_ts, bytes, &blk, vs_psola_ts_scratch_bytes(n_lanes, synth_pitch),
                             &scratch);
  if (rc != VS_OK) return rc;
  VsPtArgs a;
  memset(&a, 0, sizeof(a));
  vs_psola_common(&a.c, o.pmin, o.pmax, pcm_dev, pitch, n_lanes, marks_dev, marks_pitch, rec_dev, segs_dev, seg_pitch,
                  start_dev, start_stride, period_dev, period_stride, gain_dev, gain_stride, count_dev, count_stride,
                  target_pitch, out_dev, out_pitch, stat_dev, synth_dev, synth_pitch);
  a.out_samples = (long)out_samples;
  a.rows = (const VsPtRow *)blk.dev;
  a.map = map_dev;
  a.map_count = map_count_dev;
  a.map_pitch = (long)map_pitch;
  a.aux = (VsPtAux *)scratch.dev;
  a.unvoiced = o.unvoiced_period;
  return vs_rec_retire_both(ctx, &blk, &scratch, vs_launch_psola_ts(&a, ctx->stream));
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
  VsHostPart parts[12] = {[7] = {(void *)map, n_lanes * map_pitch * sizeof(vs_psola_anchor), VS_PART_UP, NULL},
                          {(void *)map_count, n_lanes * sizeof(int32_t), VS_PART_UP, NULL},
                          {out, n_lanes * out_samples * sizeof(int16_t), VS_PART_UP | VS_PART_DOWN, NULL},
                          {stat, n_lanes * sizeof(vs_psola_stat), VS_PART_DOWN, NULL},
                          {synth, n_lanes * synth_pitch * sizeof(vs_psola_mark), VS_PART_UP | VS_PART_DOWN, NULL}};
  vs_psola_parts(parts, n_lanes, marks, marks_pitch, rec, segs, seg_pitch, start, period, gain, count, target_pitch);
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
