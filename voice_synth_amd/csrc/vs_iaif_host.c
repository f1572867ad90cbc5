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
  if (opts) o = *opts;
  else vs_iaif_defaults(&o);
  return split_opts(&o, lpc);
}

int vs_iaif_launch(vs_ctx *ctx, const vs_iaif_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                   size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                   vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev, double *glottal_dev)
{
  vs_iaif_opts o;
  vs_lpc_opts lo;
  if (!ctx) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_iaif_defaults(&o);
  /* the arguments first, as vs_lpc_launch does (vs_lpc_rows_upload checks them again) */
  if (!pcm_dev || !fs || !frames_dev || n_lanes == 0 || n_samples == 0 || pitch < n_samples) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED;
  int rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  VsRecBlock blk;
  VsIaifArgs a;
  memset(&a, 0, sizeof(a));
  rc = vs_lpc_rows_upload(ctx, &ctx->rec_iaif, &lo, pcm_dev, pitch, n_lanes, n_samples, fs, lengths, frames_pitch,
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
  if (!ctx || !pcm || !fs || !frames || n_lanes == 0 || n_samples == 0 || pitch < n_samples || frames_pitch == 0)
    return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED;
  if (opts) o = *opts;
  else vs_iaif_defaults(&o);
  int rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  /* the pool's buffers of the host-buffer paths, as vs_lpc() uses them: the PCM in d_in; the records, the formants, the
   * coefficients and the glottal sets in d_aux */
  const size_t nfr = n_lanes * frames_pitch;
  const size_t pcm_samples = (n_lanes - 1) * pitch + n_samples;
  const size_t fr_bytes = (nfr * sizeof(vs_lpc_frame) + 255) & ~(size_t)255;
  const size_t fm_n = formants && o.n_formants > 0 ? nfr * 2 * (size_t)o.n_formants * sizeof(double) : 0;
  const size_t cf_n = coefs ? nfr * (size_t)(o.order + 1) * sizeof(double) : 0;
  const size_t gl_n = glottal ? nfr * (size_t)(o.glottal_order + 1) * sizeof(double) : 0;
  const size_t fm_bytes = (fm_n + 255) & ~(size_t)255, cf_bytes = (cf_n + 255) & ~(size_t)255;
  rc = vs_pool_device(ctx, &ctx->pool.d_in, &ctx->pool.d_in_bytes, pcm_samples * sizeof(int16_t));
  if (rc == VS_OK)
    rc = vs_pool_device(ctx, &ctx->pool.d_aux, &ctx->pool.d_aux_bytes, fr_bytes + fm_bytes + cf_bytes + gl_n);
  if (rc != VS_OK) return rc;
  char *aux = (char *)ctx->pool.d_aux;
  vs_lpc_frame *d_fr = (vs_lpc_frame *)aux;
  double *d_fm = fm_n ? (double *)(aux + fr_bytes) : NULL;
  double *d_cf = cf_n ? (double *)(aux + fr_bytes + fm_bytes) : NULL;
  double *d_gl = gl_n ? (double *)(aux + fr_bytes + fm_bytes + cf_bytes) : NULL;
  VS_HIP(ctx, hipMemcpyAsync(ctx->pool.d_in, pcm, pcm_samples * sizeof(int16_t), hipMemcpyHostToDevice, ctx->stream));
  /* what no frame covers comes back as it went */
  VS_HIP(ctx, hipMemcpyAsync(d_fr, frames, nfr * sizeof(vs_lpc_frame), hipMemcpyHostToDevice, ctx->stream));
  if (d_fm) VS_HIP(ctx, hipMemcpyAsync(d_fm, formants, fm_n, hipMemcpyHostToDevice, ctx->stream));
  if (d_cf) VS_HIP(ctx, hipMemcpyAsync(d_cf, coefs, cf_n, hipMemcpyHostToDevice, ctx->stream));
  if (d_gl) VS_HIP(ctx, hipMemcpyAsync(d_gl, glottal, gl_n, hipMemcpyHostToDevice, ctx->stream));
  rc = vs_iaif_launch(ctx, &o, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths, frames_pitch,
                      d_fr, d_fm, d_cf, d_gl);
  if (rc != VS_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  VS_HIP(ctx, hipMemcpyAsync(frames, d_fr, nfr * sizeof(vs_lpc_frame), hipMemcpyDeviceToHost, ctx->stream));
  if (d_fm) VS_HIP(ctx, hipMemcpyAsync(formants, d_fm, fm_n, hipMemcpyDeviceToHost, ctx->stream));
  if (d_cf) VS_HIP(ctx, hipMemcpyAsync(coefs, d_cf, cf_n, hipMemcpyDeviceToHost, ctx->stream));
  if (d_gl) VS_HIP(ctx, hipMemcpyAsync(glottal, d_gl, gl_n, hipMemcpyDeviceToHost, ctx->stream));
  VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VS_OK;
}
