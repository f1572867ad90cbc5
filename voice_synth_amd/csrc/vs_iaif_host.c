/*
 * vs_iaif_host.c -- host side of the IAIF analysis (include/voice_synth.h, "IAIF"): the options, their vs_lpc_opts (the
 * frame plan is the LPC analysis's, and so are the per-row records, the window tables and their upload: vs_lpc_host.c),
 * the kernel of vs_iaif.hip.  Plain C against the HIP runtime's C API, like the rest of the library's host side.
 */
#include <math.h>
#include <string.h>

#include "vs_iaif.h"
#include "vs_internal.h"

int vs_iaif_defaults(vs_iaif_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->order = VS_ORDER;
  opts->glottal_order = 4;
  opts->window = VS_LPC_HAMMING;
  opts->n_formants = 5;
  opts->window_s = 0.025;
  opts->hop_s = 0.010;
  opts->f_lo = 50.0;
  opts->leak = 0.99;
  return VS_OK;
}

/* the vs_lpc_opts of the same frames, and the checks in vs_lpc_launch's order, the IAIF ranges last */
static int split_opts(const vs_iaif_opts *o, vs_lpc_opts *lpc)
{
  memset(lpc, 0, sizeof(*lpc));
  lpc->order = o->order;
  lpc->window = o->window;
  lpc->pre_emphasis = 0;
  lpc->n_formants = o->n_formants;
  lpc->window_s = o->window_s;
  lpc->hop_s = o->hop_s;
  lpc->f_lo = o->f_lo;
  if (o->reserved_ != 0) return VS_ERR_ARG;
  const int rc = vs_lpc_check_opts(lpc);
  if (rc != VS_OK) return rc;
  if (o->glottal_order < 1 || o->glottal_order > o->order) return VS_ERR_RANGE;
  if (!(o->leak >= 0.0 && o->leak <= 1.0)) return VS_ERR_RANGE; /* NaN included */
  return VS_OK;
}

int vs_iaif_lpc_opts(const vs_iaif_opts *opts, vs_lpc_opts *lpc)
{
  vs_iaif_opts o;
  if (!lpc) return VS_ERR_ARG;
  VS_OPTS_OR(o, opts, vs_iaif_defaults);
  return split_opts(&o, lpc);
}

int vs_iaif_launch(vs_ctx *ctx, const vs_iaif_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                   size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                   vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev, double *glottal_dev)
{
  vs_iaif_opts o;
  vs_lpc_opts lo;
  /* the arguments first, as vs_lpc_launch does (vs_lpc_rows_upload checks them again) */
  int rc = vs_frame_check(ctx, pcm_dev, pitch, n_lanes, n_samples, fs, frames_pitch, frames_dev, 0);
  if (rc != VS_OK) return rc;
  VS_OPTS_OR(o, opts, vs_iaif_defaults);
  rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  VsRecBlock blk;
  VsIaifArgs a;
  memset(&a, 0, sizeof(a));
  rc = vs_lpc_rows_upload(ctx, &ctx->rec_iaif, &lo, 0, pcm_dev, pitch, n_lanes, n_samples, fs, lengths, frames_pitch,
                          frames_dev, formants_dev, coefs_dev, &blk, &a.lpc);
  if (rc != VS_OK) return rc;
  a.glottal = glottal_dev;
  a.glottal_order = o.glottal_order;
  a.leak = o.leak;
  return vs_rec_retire(ctx, &blk, vs_launch_iaif(&a, ctx->stream));
}

int vs_iaif(vs_ctx *ctx, const vs_iaif_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
            const int32_t *fs, const int32_t *lengths, size_t frames_pitch, vs_lpc_frame *frames, double *formants,
            double *coefs, double *glottal)
{
  vs_iaif_opts o;
  vs_lpc_opts lo;
  int rc = vs_frame_check(ctx, pcm, pitch, n_lanes, n_samples, fs, frames_pitch, frames, 1);
  if (rc != VS_OK) return rc;
  VS_OPTS_OR(o, opts, vs_iaif_defaults);
  rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  /* as vs_lpc(): the PCM in d_in; the records, the formants, the coefficients and the glottal sets go up and come back */
  const size_t nfr = n_lanes * frames_pitch;
  VsHostPart parts[4];
  vs_frame_parts(parts, nfr, o.order, o.n_formants, frames, formants, coefs);
  parts[3] = (VsHostPart){glottal, nfr * (size_t)(o.glottal_order + 1) * sizeof(double), VS_PART_UP | VS_PART_DOWN, NULL};
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 4);
  if (rc != VS_OK) return rc;
  rc = vs_iaif_launch(ctx, &o, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths, frames_pitch,
                      (vs_lpc_frame *)parts[0].dev, (double *)parts[1].dev, (double *)parts[2].dev,
                      (double *)parts[3].dev);
  return vs_host_end(ctx, rc, parts, 4);
}
