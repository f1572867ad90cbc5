/*
 * vs_guided_host.c -- host side of the guided marks (include/voice_synth.h, "guided marks"): the options, the lag
 * bounds, hop, frames and centre offset of every row, the upload of the per-row records, the plan kernel's scratch, the
 * two kernels of vs_guided.hip.  Plain C against the HIP runtime's C API, like the rest of the library's host side.
 * The option checks and the row plan touch no device: vs_guided_plan is their public face.
 */
#include <math.h>
#include <string.h>

#include "vs_guided.h"
#include "vs_internal.h"

int vs_guided_defaults(vs_guided_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->f0_min = 50.0f;
  opts->f0_max = 500.0f;
  opts->polarity = 1;
  opts->segments = VS_MG_ALL;
  opts->edge_frames = 1;
  opts->min_frames = 3;
  opts->hop_s = 0.010;
  return VS_OK;
}

/* every VS_ERR_ARG of the options, then their VS_ERR_RANGE */
static int check_opts(const vs_guided_opts *o)
{
  if (!(o->f0_min > 0.0f) || !(o->f0_max > 0.0f) || !isfinite(o->f0_min) || !isfinite(o->f0_max)) return VS_ERR_ARG;
  if (!isfinite(o->hop_s) || o->hop_s < 0.0) return VS_ERR_ARG;
  if (o->polarity != 1 && o->polarity != -1) return VS_ERR_ARG;
  if (o->segments != VS_MG_ALL && o->segments != VS_MG_LONGEST) return VS_ERR_ARG;
  if (o->edge_frames < 0 || o->edge_frames > VS_MG_MAX_EDGE || o->min_frames < 1) return VS_ERR_RANGE;
  return VS_OK;
}

/* one row's record (the pitch track's formulas, in double); VS_ERR_RANGE outside the limits */
static int row_plan(int32_t fs, int32_t len, const vs_guided_opts *o, VsMgRow *r)
{
  if (fs <= 0 || len < 0) return VS_ERR_RANGE;
  const double lo = floor((double)fs / (double)o->f0_max), hi = ceil((double)fs / (double)o->f0_min);
  if (!(lo >= 2.0) || !(hi <= (double)VS_AC_MAX_LAG) || !(lo < hi)) return VS_ERR_RANGE;
  const double H = floor(o->hop_s * (double)fs + 0.5);
  if (!(H >= 1.0) || !(H <= 2147483647.0)) return VS_ERR_RANGE;
  r->len = len;
  r->fs = fs;
  r->tmin = (int32_t)lo;
  r->tmax = (int32_t)hi;
  r->H = (int32_t)H;
  const int32_t need = 3 * r->tmax + 2;
  r->n_frames = len >= need ? 1 + (len - need) / r->H : 0;
  r->C = r->tmax + r->tmax / 2;
  r->reserved_ = 0;
  return VS_OK;
}

int vs_guided_plan(const vs_guided_opts *opts, int32_t fs, int32_t len, int32_t *tmin, int32_t *tmax, int32_t *hop,
                   int32_t *n_frames, int32_t *centre)
{
  vs_guided_opts o;
  VsMgRow r;
  if (opts) o = *opts;
  else vs_guided_defaults(&o);
  int rc = check_opts(&o);
  if (rc != VS_OK) return rc;
  rc = row_plan(fs, len, &o, &r);
  if (rc != VS_OK) return rc;
  if (tmin) *tmin = r.tmin;
  if (tmax) *tmax = r.tmax;
  if (hop) *hop = r.H;
  if (n_frames) *n_frames = r.n_frames;
  if (centre) *centre = r.C;
  return VS_OK;
}

/* what vs_guided_launch and vs_guided check alike: every VS_ERR_ARG before any VS_ERR_UNSUPPORTED */
static int check_args(const vs_ctx *ctx, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
                      const int32_t *fs, size_t frames_pitch, const vs_acoustic *out, const int32_t *marks,
                      size_t marks_pitch, const vs_guided_rec *rec, const vs_guided_seg *segs, size_t seg_pitch)
{
  if (!ctx || !pcm || !fs || !out || !rec || n_lanes == 0 || n_samples == 0 || pitch < n_samples || frames_pitch == 0)
    return VS_ERR_ARG;
  if ((marks && marks_pitch == 0) || (segs && seg_pitch == 0)) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu || marks_pitch > 0x7FFFFFFFu ||
      seg_pitch > 0x7FFFFFFFu)
    return VS_ERR_UNSUPPORTED;
  return VS_OK;
}

int vs_guided_launch(vs_ctx *ctx, const vs_guided_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                     size_t n_samples, const int32_t *fs, const int32_t *lengths, const vs_pitch_frame *frames_dev,
                     size_t frames_pitch, vs_acoustic *out_dev, int32_t *marks_dev, size_t marks_pitch,
                     vs_guided_rec *rec_dev, vs_guided_seg *segs_dev, size_t seg_pitch)
{
  vs_guided_opts o;
  int rc = check_args(ctx, pcm_dev, pitch, n_lanes, n_samples, fs, frames_pitch, out_dev, marks_dev, marks_pitch, rec_dev,
                      segs_dev, seg_pitch);
  if (rc != VS_OK) return rc;
  if (!frames_dev || ((uintptr_t)frames_dev & 7) != 0) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_guided_defaults(&o);
  rc = check_opts(&o);
  if (rc != VS_OK) return rc;

  const size_t bytes = n_lanes * sizeof(VsMgRow);
  void *host = NULL;
  rc = vs_rec_stage(ctx, &ctx->rec_guided, bytes, &host);
  if (rc != VS_OK) return rc;
  VsMgRow *rows = (VsMgRow *)host;
  for (size_t i = 0; i < n_lanes; i++) {
    const int32_t len = lengths ? lengths[i] : (int32_t)n_samples;
    if (len < 0 || (size_t)len > n_samples) return VS_ERR_ARG;
    rc = row_plan(fs[i], len, &o, &rows[i]);
    if (rc != VS_OK) return rc;
    if ((size_t)rows[i].n_frames > frames_pitch) return VS_ERR_RANGE;
  }

  /* the plan kernel's scratch: a block of the same cache, retired behind the same kernels */
  VsRecBlock blk, scratch;
  rc = vs_rec_upload_scratch(ctx, &ctx->rec_guided, bytes, &blk, vs_mg_scratch_bytes(n_lanes, frames_pitch), &scratch);
  if (rc != VS_OK) return rc;
  VsMgArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm_dev;
  a.pitch = (long)pitch;
  a.n_lanes = (long)n_lanes;
  a.n_samples = (long)n_samples;
  a.rows = (const VsMgRow *)blk.dev;
  a.frames = frames_dev;
  a.frames_pitch = (long)frames_pitch;
  a.head = (VsMgHead *)scratch.dev;
  a.lag = (int32_t *)((char *)scratch.dev + n_lanes * sizeof(VsMgHead));
  a.link = a.lag + n_lanes * frames_pitch;
  a.out = out_dev;
  a.marks = marks_dev;
  a.marks_pitch = marks_dev ? (long)marks_pitch : 0;
  a.rec = rec_dev;
  a.segs = segs_dev;
  a.seg_pitch = segs_dev ? (long)seg_pitch : 0;
  a.polarity = o.polarity;
  a.segments = o.segments;
  a.edge_frames = o.edge_frames;
  a.min_frames = o.min_frames;
  return vs_rec_retire_both(ctx, &blk, &scratch, vs_launch_guided(&a, ctx->stream));
}

int vs_guided(vs_ctx *ctx, const vs_guided_opts *opts, const vs_pitch_opts *pitch_opts, const int16_t *pcm, size_t pitch,
              size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
              vs_pitch_frame *frames, vs_acoustic *out, int32_t *marks, size_t marks_pitch, vs_guided_rec *rec,
              vs_guided_seg *segs, size_t seg_pitch)
{
  vs_guided_opts o;
  vs_pitch_opts po;
  int rc = check_args(ctx, pcm, pitch, n_lanes, n_samples, fs, frames_pitch, out, marks, marks_pitch, rec, segs, seg_pitch);
  if (rc != VS_OK) return rc;
  if (frames && ((uintptr_t)frames & 7) != 0) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_guided_defaults(&o);
  rc = check_opts(&o);
  if (rc != VS_OK) return rc;
  if (pitch_opts) po = *pitch_opts;
  else vs_pitch_defaults(&po);
  po.f0_min = o.f0_min;
  po.f0_max = o.f0_max;
  po.hop_s = o.hop_s;

  /* the PCM in d_in; the track's records go up and come back when the caller keeps them, else they live in a block of
   * the retired-block cache; the marks are filled with -1; the segment records go up, so that the slots past a row's
   * runs come back as they went */
  const size_t frame_bytes = n_lanes * frames_pitch * sizeof(vs_pitch_frame);
  VsHostPart parts[5] = {{out, n_lanes * sizeof(vs_acoustic), VS_PART_DOWN, NULL},
                         {marks, n_lanes * marks_pitch * sizeof(int32_t), VS_PART_FILL_FF | VS_PART_DOWN, NULL},
                         {rec, n_lanes * sizeof(vs_guided_rec), VS_PART_DOWN, NULL},
                         {segs, n_lanes * seg_pitch * sizeof(vs_guided_seg), VS_PART_UP | VS_PART_DOWN, NULL},
                         {frames, frame_bytes, VS_PART_UP | VS_PART_DOWN, NULL}};
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 5);
  if (rc != VS_OK) return rc;
  VsRecBlock own;
  own.dev = NULL;
  own.cap = 0;
  vs_pitch_frame *frames_dev = (vs_pitch_frame *)parts[4].dev;
  if (!frames_dev) {
    const hipError_t e = plan_block_get(ctx, frame_bytes, &own.dev, &own.cap);
    if (e != hipSuccess) {
      ctx->last_hip_error = (int)e;
      return vs_host_end(ctx, VS_ERR_HIP, parts, 5);
    }
    frames_dev = (vs_pitch_frame *)own.dev;
  }
  const int16_t *pcm_dev = (const int16_t *)ctx->pool.d_in;
  rc = vs_pitch_launch(ctx, &po, pcm_dev, pitch, n_lanes, n_samples, fs, lengths, frames_pitch, frames_dev);
  if (rc == VS_OK)
    rc = vs_guided_launch(ctx, &o, pcm_dev, pitch, n_lanes, n_samples, fs, lengths, frames_dev, frames_pitch,
                          (vs_acoustic *)parts[0].dev, (int32_t *)parts[1].dev, marks_pitch,
                          (vs_guided_rec *)parts[2].dev, (vs_guided_seg *)parts[3].dev, seg_pitch);
  if (own.dev) { /* behind whatever was enqueued; after a refusal nothing reads it */
    const int rc2 = vs_rec_retire(ctx, &own, hipSuccess);
    if (rc == VS_OK) rc = rc2;
  }
  return vs_host_end(ctx, rc, parts, 5);
}
