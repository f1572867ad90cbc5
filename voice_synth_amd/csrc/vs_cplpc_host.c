/*
 * vs_cplpc_host.c -- host side of the closed-phase covariance LPC (include/voice_synth.h, "closed-phase covariance LPC"):
 * the options, their vs_lpc_opts (with window_s > 0 the frame plan is the LPC analysis's, and so are the per-row records
 * and their upload: vs_lpc_host.c; with window_s == 0 a row's record is one frame over the whole row, through the same
 * record-upload path), the kernel of vs_cplpc.hip.  Plain C against the HIP runtime's C API, like the rest of the
 * library's host side.
 */
#include <math.h>
#include <string.h>

#include "vs_cplpc.h"
#include "vs_internal.h"

int vs_cplpc_defaults(vs_cplpc_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->order = VS_ORDER;
  opts->anchor = VS_CP_ANCHOR_CLOSE;
  opts->delay = 4;
  opts->span_q = 77;
  opts->min_equations = 0;
  opts->n_formants = 5;
  opts->window_s = 0.0;
  opts->hop_s = 0.010;
  opts->f_lo = 50.0;
  return VS_OK;
}

/* the vs_lpc_opts of the same frames, and the checks in vs_lpc_launch's order, the closed-phase ranges last */
static int split_opts(const vs_cplpc_opts *o, vs_lpc_opts *lpc)
{
  memset(lpc, 0, sizeof(*lpc));
  lpc->order = o->order;
  lpc->window = VS_LPC_RECTANGULAR;
  lpc->pre_emphasis = 0;
  lpc->n_formants = o->n_formants;
  lpc->window_s = o->window_s;
  lpc->hop_s = o->hop_s;
  lpc->f_lo = o->f_lo;
  if (o->reserved_ != 0) return VS_ERR_ARG;
  const int rc = vs_lpc_check_opts(lpc);
  if (rc != VS_OK) return rc;
  if (o->window_s < 0.0) return VS_ERR_RANGE; /* as vs_lpc_launch answers a window no frame fits */
  if (o->anchor != VS_CP_ANCHOR_CLOSE && o->anchor != VS_CP_ANCHOR_GCI && o->anchor != VS_CP_ANCHOR_PEAK) return VS_ERR_RANGE;
  if (o->delay < -32768 || o->delay > 32767 || o->span_q < 1 || o->span_q > 256) return VS_ERR_RANGE;
  if (o->min_equations != 0 && o->min_equations < o->order) return VS_ERR_RANGE;
  return VS_OK;
}

int vs_cplpc_lpc_opts(const vs_cplpc_opts *opts, vs_lpc_opts *lpc)
{
  vs_cplpc_opts o;
  if (!lpc) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_cplpc_defaults(&o);
  return split_opts(&o, lpc);
}

int vs_cplpc_frames(const vs_cplpc_opts *opts, int32_t fs, int32_t len, int32_t *n_frames)
{
  vs_cplpc_opts o;
  vs_lpc_opts lo;
  if (!n_frames) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_cplpc_defaults(&o);
  const int rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  if (o.window_s > 0.0) return vs_lpc_frames(&lo, fs, len, n_frames);
  if (fs <= 0 || len < 0) return VS_ERR_RANGE;
  *n_frames = 1;
  return VS_OK;
}

/* window_s == 0: the arguments as vs_lpc_rows_upload checks them, and one record per row -- one frame [0, len) */
static int whole_rows_upload(vs_ctx *ctx, VsRecSlot *slot, const vs_lpc_opts *o, const int16_t *pcm_dev, size_t pitch,
                             size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths,
                             size_t frames_pitch, vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev,
                             VsRecBlock *blk, VsLpcArgs *args)
{
  for (size_t i = 0; i < n_lanes; i++) {
    const int32_t len = lengths ? lengths[i] : (int32_t)n_samples;
    if (len < 0 || (size_t)len > n_samples) return VS_ERR_ARG;
    if (fs[i] <= 0) return VS_ERR_RANGE;
  }
  const size_t bytes = n_lanes * sizeof(VsLpcRow);
  void *host = NULL;
  int rc = vs_rec_stage(ctx, slot, bytes, &host);
  if (rc != VS_OK) return rc;
  VsLpcRow *rows = (VsLpcRow *)host;
  for (size_t i = 0; i < n_lanes; i++) {
    memset(&rows[i], 0, sizeof(rows[i]));
    rows[i].first = (int64_t)i;
    rows[i].fs = fs[i];
    rows[i].L = lengths ? lengths[i] : (int32_t)n_samples;
    rows[i].n_frames = 1;
  }
  rc = vs_rec_upload(ctx, slot, bytes, blk);
  if (rc != VS_OK) return rc;
  memset(args, 0, sizeof(*args));
  args->pcm = pcm_dev;
  args->pitch = (long)pitch;
  args->n_lanes = (long)n_lanes;
  args->total_frames = (long)n_lanes;
  args->rows = (const VsLpcRow *)blk->dev;
  args->frames = frames_dev;
  args->formants = formants_dev;
  args->coefs = coefs_dev;
  args->frames_pitch = (long)frames_pitch;
  args->order = o->order;
  args->n_formants = o->n_formants;
  args->f_lo = o->f_lo;
  return VS_OK;
}

int vs_cplpc_launch(vs_ctx *ctx, const vs_cplpc_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                    size_t n_samples, const int32_t *fs, const int32_t *lengths, const vs_glottal_rec *glottal_dev,
                    const vs_glottal_cycle *cycles_dev, size_t cycles_pitch, size_t frames_pitch,
                    vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev, int32_t *counts_dev)
{
  vs_cplpc_opts o;
  vs_lpc_opts lo;
  if (!ctx) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_cplpc_defaults(&o);
  /* the arguments first, as vs_lpc_launch does (vs_lpc_rows_upload checks its own again) */
  if (!pcm_dev || !fs || !frames_dev || !glottal_dev || !cycles_dev || n_lanes == 0 || n_samples == 0 ||
      pitch < n_samples || cycles_pitch == 0 || frames_pitch == 0)
    return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu || cycles_pitch > 0x7FFFFFFFu)
    return VS_ERR_UNSUPPORTED;
  int rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  VsRecBlock blk;
  VsCplpcArgs a;
  memset(&a, 0, sizeof(a));
  rc = (o.window_s > 0.0 ? vs_lpc_rows_upload : whole_rows_upload)(ctx, &ctx->rec_cplpc, &lo, pcm_dev, pitch, n_lanes,
                                                                   n_samples, fs, lengths, frames_pitch, frames_dev,
                                                                   formants_dev, coefs_dev, &blk, &a.lpc);
  if (rc != VS_OK) return rc;
  a.glottal = glottal_dev;
  a.cycles = cycles_dev;
  a.cycles_pitch = (long)cycles_pitch;
  a.counts = counts_dev;
  a.anchor = o.anchor;
  a.delay = o.delay;
  a.span_q = o.span_q;
  a.min_equations = o.min_equations;
  return vs_rec_retire(ctx, &blk, vs_launch_cplpc(&a, ctx->stream));
}

int vs_cplpc(vs_ctx *ctx, const vs_cplpc_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
             const int32_t *fs, const int32_t *lengths, const vs_glottal_rec *glottal, const vs_glottal_cycle *cycles,
             size_t cycles_pitch, size_t frames_pitch, vs_lpc_frame *frames, double *formants, double *coefs,
             int32_t *counts)
{
  vs_cplpc_opts o;
  vs_lpc_opts lo;
  if (!ctx || !pcm || !fs || !frames || !glottal || !cycles || n_lanes == 0 || n_samples == 0 || pitch < n_samples ||
      frames_pitch == 0 || cycles_pitch == 0)
    return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu || cycles_pitch > 0x7FFFFFFFu)
    return VS_ERR_UNSUPPORTED;
  if (opts) o = *opts;
  else vs_cplpc_defaults(&o);
  int rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  /* as vs_lpc(): the PCM in d_in; the row and cycle records go up, the four outputs go up and come back */
  const size_t nfr = n_lanes * frames_pitch;
  const unsigned both = VS_PART_UP | VS_PART_DOWN;
  VsHostPart parts[6] = {{(void *)glottal, n_lanes * sizeof(vs_glottal_rec), VS_PART_UP, NULL},
                         {(void *)cycles, n_lanes * cycles_pitch * sizeof(vs_glottal_cycle), VS_PART_UP, NULL},
                         {frames, nfr * sizeof(vs_lpc_frame), both, NULL},
                         {formants, nfr * 2 * (size_t)o.n_formants * sizeof(double), both, NULL},
                         {coefs, nfr * (size_t)(o.order + 1) * sizeof(double), both, NULL},
                         {counts, nfr * 2 * sizeof(int32_t), both, NULL}};
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 6);
  if (rc != VS_OK) return rc;
  rc = vs_cplpc_launch(ctx, &o, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths,
                       (const vs_glottal_rec *)parts[0].dev, (const vs_glottal_cycle *)parts[1].dev, cycles_pitch,
                       frames_pitch, (vs_lpc_frame *)parts[2].dev, (double *)parts[3].dev, (double *)parts[4].dev,
                       (int32_t *)parts[5].dev);
  return vs_host_end(ctx, rc, parts, 6);
}
