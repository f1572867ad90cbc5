/*
 * vs_cplpc_host.c -- host side of the closed-phase covariance LPC (include/voice_synth.h, "closed-phase covariance LPC"):
 * the options, their vs_lpc_opts (with window_s > 0 the frame plan is the LPC analysis's, and so are the per-row records
 * and their upload: vs_lpc_host.c; with window_s == 0 a row's record is one frame over the whole row, the same upload's
 * whole-row plan), the kernel of vs_cplpc.hip.  Plain C against the HIP runtime's C API, like the rest of the
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
  VS_OPTS_OR(o, opts, vs_cplpc_defaults);
  return split_opts(&o, lpc);
}

int vs_cplpc_frames(const vs_cplpc_opts *opts, int32_t fs, int32_t len, int32_t *n_frames)
{
  vs_cplpc_opts o;
  vs_lpc_opts lo;
  if (!n_frames) return VS_ERR_ARG;
  VS_OPTS_OR(o, opts, vs_cplpc_defaults);
  const int rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  if (o.window_s > 0.0) return vs_lpc_frames(&lo, fs, len, n_frames);
  VsLpcRow r;
  const int rrc = vs_lpc_row_whole(fs, len, &r);
  if (rrc == VS_OK) *n_frames = r.n_frames;
  return rrc;
}

/* vs_frame_check with frames_pitch > 0, and the cycle records: every VS_ERR_ARG before any VS_ERR_UNSUPPORTED */
static int check_args(const vs_ctx *ctx, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
                      const int32_t *fs, const vs_glottal_rec *glottal, const vs_glottal_cycle *cycles,
                      size_t cycles_pitch, size_t frames_pitch, const vs_lpc_frame *frames)
{
  if (!glottal || !cycles || cycles_pitch == 0) return VS_ERR_ARG;
  const int rc = vs_frame_check(ctx, pcm, pitch, n_lanes, n_samples, fs, frames_pitch, frames, 1);
  return rc == VS_OK && cycles_pitch > 0x7FFFFFFFu ? VS_ERR_UNSUPPORTED : rc;
}

int vs_cplpc_launch(vs_ctx *ctx, const vs_cplpc_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                    size_t n_samples, const int32_t *fs, const int32_t *lengths, const vs_glottal_rec *glottal_dev,
                    const vs_glottal_cycle *cycles_dev, size_t cycles_pitch, size_t frames_pitch,
                    vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev, int32_t *counts_dev)
{
  vs_cplpc_opts o;
  vs_lpc_opts lo;
  /* the arguments first, as vs_lpc_launch does (vs_lpc_rows_upload checks its own again) */
  int rc = check_args(ctx, pcm_dev, pitch, n_lanes, n_samples, fs, glottal_dev, cycles_dev, cycles_pitch, frames_pitch,
                      frames_dev);
  if (rc != VS_OK) return rc;
  VS_OPTS_OR(o, opts, vs_cplpc_defaults);
  rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  VsRecBlock blk;
  VsCplpcArgs a;
  memset(&a, 0, sizeof(a));
  rc = vs_lpc_rows_upload(ctx, &ctx->rec_cplpc, &lo, !(o.window_s > 0.0), pcm_dev, pitch, n_lanes, n_samples, fs, lengths,
                          frames_pitch, frames_dev, formants_dev, coefs_dev, &blk, &a.lpc);
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
  int rc = check_args(ctx, pcm, pitch, n_lanes, n_samples, fs, glottal, cycles, cycles_pitch, frames_pitch, frames);
  if (rc != VS_OK) return rc;
  VS_OPTS_OR(o, opts, vs_cplpc_defaults);
  rc = split_opts(&o, &lo);
  if (rc != VS_OK) return rc;
  /* as vs_lpc(): the PCM in d_in; the row and cycle records go up, the four outputs go up and come back */
  const size_t nfr = n_lanes * frames_pitch;
  VsHostPart parts[6] = {{(void *)glottal, n_lanes * sizeof(vs_glottal_rec), VS_PART_UP, NULL},
                         {(void *)cycles, n_lanes * cycles_pitch * sizeof(vs_glottal_cycle), VS_PART_UP, NULL}};
  vs_frame_parts(parts + 2, nfr, o.order, o.n_formants, frames, formants, coefs);
  parts[5] = (VsHostPart){counts, nfr * 2 * sizeof(int32_t), VS_PART_UP | VS_PART_DOWN, NULL};
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 6);
  if (rc != VS_OK) return rc;
  rc = vs_cplpc_launch(ctx, &o, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths,
                       (const vs_glottal_rec *)parts[0].dev, (const vs_glottal_cycle *)parts[1].dev, cycles_pitch,
                       frames_pitch, (vs_lpc_frame *)parts[2].dev, (double *)parts[3].dev, (double *)parts[4].dev,
                       (int32_t *)parts[5].dev);
  return vs_host_end(ctx, rc, parts, 6);
}
