/*
 * vs_glottal_host.c -- host side of the glottal parameters (include/voice_synth.h, "glottal parameters"): the options,
 * the launch of vs_glottal.hip's kernel behind the measurement, the host-buffer call that chains the two.
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.
 */
#include <string.h>

#include "vs_glottal.h"
#include "vs_internal.h"

int vs_glottal_defaults(vs_glottal_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  opts->level_open = 26; /* 10 % of the amplitude */
  opts->level_mid = 128; /* 50 %: QOQ */
  opts->polarity = 1;
  opts->reserved_ = 0;
  return VS_OK;
}

static int check_opts(const vs_glottal_opts *o)
{
  if ((o->polarity != 1 && o->polarity != -1) || o->reserved_ != 0) return VS_ERR_ARG;
  if (o->level_open < 0 || o->level_open > 255 || o->level_mid < o->level_open || o->level_mid > 255) return VS_ERR_RANGE;
  return VS_OK;
}

/* the sizes the launch and the host-buffer call check alike (the kernel's int arithmetic steps 64 past a sample index) */
static int check_sizes(size_t pitch, size_t n_lanes, size_t n_samples, size_t marks_pitch, const void *cycles,
                       size_t cycles_pitch)
{
  if (n_lanes == 0 || n_samples == 0 || pitch < n_samples || marks_pitch == 0) return VS_ERR_ARG;
  if (cycles && cycles_pitch == 0) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples >= 0x7FFFFFFFu - 256u || marks_pitch >= 0x7FFFFFFFu - 256u ||
      cycles_pitch > 0x7FFFFFFFu)
    return VS_ERR_UNSUPPORTED;
  return VS_OK;
}

int vs_glottal_launch(vs_ctx *ctx, const vs_glottal_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                      size_t n_samples, const vs_acoustic *meas_dev, const int32_t *marks_dev, size_t marks_pitch,
                      vs_glottal_rec *out_dev, vs_glottal_cycle *cycles_dev, size_t cycles_pitch)
{
  vs_glottal_opts o;
  if (!ctx || !pcm_dev || !meas_dev || !marks_dev || !out_dev) return VS_ERR_ARG;
  int rc = check_sizes(pitch, n_lanes, n_samples, marks_pitch, cycles_dev, cycles_pitch);
  if (rc != VS_OK) return rc;
  if (opts) o = *opts;
  else vs_glottal_defaults(&o);
  rc = check_opts(&o);
  if (rc != VS_OK) return rc;

  VsGlArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm_dev;
  a.pitch = (long)pitch;
  a.n_lanes = (long)n_lanes;
  a.n_samples = (int)n_samples;
  a.marks_pitch = (int)marks_pitch;
  a.meas = meas_dev;
  a.marks = marks_dev;
  a.out = out_dev;
  a.cycles = cycles_dev;
  a.cycles_pitch = cycles_dev ? (long)cycles_pitch : 0;
  a.level_open = o.level_open;
  a.level_mid = o.level_mid;
  a.polarity = o.polarity;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, vs_launch_glottal(&a, ctx->stream));
  return VS_OK;
}

int vs_glottal(vs_ctx *ctx, const vs_measure_opts *mopts, const vs_glottal_opts *gopts, const int16_t *pcm, size_t pitch,
               size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t marks_pitch,
               vs_acoustic *meas, int32_t *marks, vs_glottal_rec *out, vs_glottal_cycle *cycles, size_t cycles_pitch)
{
  vs_measure_opts mo;
  vs_glottal_opts go;
  if (!ctx || !pcm || !fs || !meas || !marks || !out) return VS_ERR_ARG;
  int rc = check_sizes(pitch, n_lanes, n_samples, marks_pitch, cycles, cycles_pitch);
  if (rc != VS_OK) return rc;
  if (mopts) mo = *mopts;
  else vs_measure_defaults(&mo);
  if (gopts) go = *gopts;
  else vs_glottal_defaults(&go);
  rc = check_opts(&go);
  if (rc != VS_OK) return rc;
  if (mo.polarity != go.polarity) return VS_ERR_ARG;
  /* the PCM in d_in; records and marks (filled with -1 past the last mark) come back, the cycle records go up first so
   * that the slots no cycle fills come back as they were */
  VsHostPart parts[4] = {{meas, n_lanes * sizeof(vs_acoustic), VS_PART_DOWN, NULL},
                         {marks, n_lanes * marks_pitch * sizeof(int32_t), VS_PART_FILL_FF | VS_PART_DOWN, NULL},
                         {out, n_lanes * sizeof(vs_glottal_rec), VS_PART_DOWN, NULL},
                         {cycles, n_lanes * cycles_pitch * sizeof(vs_glottal_cycle), VS_PART_UP | VS_PART_DOWN, NULL}};
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 4);
  if (rc != VS_OK) return rc;
  rc = vs_measure_launch(ctx, &mo, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths,
                         (vs_acoustic *)parts[0].dev, (int32_t *)parts[1].dev, marks_pitch);
  if (rc == VS_OK)
    rc = vs_glottal_launch(ctx, &go, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples,
                           (const vs_acoustic *)parts[0].dev, (const int32_t *)parts[1].dev, marks_pitch,
                           (vs_glottal_rec *)parts[2].dev, (vs_glottal_cycle *)parts[3].dev, cycles_pitch);
  return vs_host_end(ctx, rc, parts, 4);
}
