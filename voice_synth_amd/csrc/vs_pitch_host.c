/*
 * vs_pitch_host.c -- host side of the pitch track (include/voice_synth.h, "pitch track"): the options, the lag bounds,
 * hop and frames of every row, the Lg table, the upload of the per-row records with the table behind them, the two
 * kernels of vs_pitch.hip.  Plain C against the HIP runtime's C API, like the rest of the library's host side.
 */
#include <math.h>
#include <string.h>

#include "vs_internal.h"
#include "vs_pitch.h"

int vs_pitch_defaults(vs_pitch_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->f0_min = 50.0f;
  opts->f0_max = 500.0f;
  opts->voicing_q = 14746; /* Praat's "To Pitch (ac)" defaults, in Q15: 0.45, 0.01, 0.35, 0.14 */
  opts->octave_q = 328;
  opts->jump_q = 11469;
  opts->vuv_q = 4588;
  opts->silence_rms = 16;
  opts->hop_s = 0.010;
  return VS_OK;
}

static int cost_ok(int32_t v) { return v >= 0 && v <= VS_PT_MAX_COST; }

static int check_opts(const vs_pitch_opts *o)
{
  if (!(o->f0_min > 0.0f) || !(o->f0_max > 0.0f) || !isfinite(o->f0_min) || !isfinite(o->f0_max)) return VS_ERR_ARG;
  if (!isfinite(o->hop_s) || o->hop_s < 0.0 || o->reserved_ != 0) return VS_ERR_ARG;
  if (!cost_ok(o->voicing_q) || !cost_ok(o->octave_q) || !cost_ok(o->jump_q) || !cost_ok(o->vuv_q)) return VS_ERR_ARG;
  if (o->silence_rms < 0 || o->silence_rms > 32767) return VS_ERR_ARG;
  return VS_OK;
}

/* one row's record but for `first` (the header's formulas, in double); VS_ERR_RANGE outside the limits */
static int row_plan(int32_t fs, int32_t len, const vs_pitch_opts *o, VsPtRow *r)
{
  if (fs <= 0 || len < 0) return VS_ERR_RANGE;
  const double lo = floor((double)fs / (double)o->f0_max), hi = ceil((double)fs / (double)o->f0_min);
  if (!(lo >= 2.0) || !(hi <= (double)VS_AC_MAX_LAG) || !(lo < hi)) return VS_ERR_RANGE;
  const double H = floor(o->hop_s * (double)fs + 0.5);
  if (!(H >= 1.0) || !(H <= 2147483647.0)) return VS_ERR_RANGE;
  r->first = 0;
  r->len = len;
  r->fs = fs;
  r->tmin = (int32_t)lo;
  r->tmax = (int32_t)hi;
  r->H = (int32_t)H;
  const int32_t need = 3 * r->tmax + 2;
  r->n_frames = len >= need ? 1 + (len - need) / r->H : 0;
  return VS_OK;
}

int vs_pitch_frames(const vs_pitch_opts *opts, int32_t fs, int32_t len, int32_t *n_frames)
{
  vs_pitch_opts o;
  VsPtRow r;
  if (!n_frames) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_pitch_defaults(&o);
  int rc = check_opts(&o);
  if (rc != VS_OK) return rc;
  rc = row_plan(fs, len, &o, &r);
  if (rc == VS_OK) *n_frames = r.n_frames;
  return rc;
}

int vs_pitch_log2_table(int32_t n, int32_t *lg)
{
  if (!lg || n < 1 || n > VS_AC_MAX_LAG + 1) return VS_ERR_ARG;
  lg[0] = 0;
  for (int32_t t = 1; t < n; t++) lg[t] = (int32_t)floor(256.0 * log2((double)t) + 0.5);
  return VS_OK;
}

/* what vs_pitch_launch and vs_pitch check alike: every VS_ERR_ARG before any VS_ERR_UNSUPPORTED */
static int check_args(const vs_ctx *ctx, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
                      const int32_t *fs, size_t frames_pitch, const vs_pitch_frame *frames)
{
  if (!ctx || !pcm || !fs || !frames || n_lanes == 0 || n_samples == 0 || pitch < n_samples || frames_pitch == 0) return VS_ERR_ARG;
  if (((uintptr_t)frames & 7) != 0) return VS_ERR_ARG; /* the records hold an int64 */
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED;
  return VS_OK;
}

int vs_pitch_launch(vs_ctx *ctx, const vs_pitch_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                    size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                    vs_pitch_frame *frames_dev)
{
  vs_pitch_opts o;
  int rc = check_args(ctx, pcm_dev, pitch, n_lanes, n_samples, fs, frames_pitch, frames_dev);
  if (rc != VS_OK) return rc;
  if (opts) o = *opts;
  else vs_pitch_defaults(&o);
  rc = check_opts(&o);
  if (rc != VS_OK) return rc;

  /* the rows, and behind them Lg[0 .. VS_AC_MAX_LAG] */
  const size_t row_bytes = n_lanes * sizeof(VsPtRow), bytes = row_bytes + (VS_AC_MAX_LAG + 1) * sizeof(int32_t);
  void *host = NULL;
  rc = vs_rec_stage(ctx, &ctx->rec_pitch, bytes, &host);
  if (rc != VS_OK) return rc;
  VsPtRow *rows = (VsPtRow *)host;
  int lds = 0;
  int64_t total = 0;
  for (size_t i = 0; i < n_lanes; i++) {
    VsPtRow *r = &rows[i];
    const int32_t len = lengths ? lengths[i] : (int32_t)n_samples;
    if (len < 0 || (size_t)len > n_samples) return VS_ERR_ARG;
    rc = row_plan(fs[i], len, &o, r);
    if (rc != VS_OK) return rc;
    if ((size_t)r->n_frames > frames_pitch) return VS_ERR_RANGE;
    r->first = total;
    total += r->n_frames;
    const int l = vs_pt_lds_doubles(r->tmin, r->tmax);
    if (l > lds) lds = l;
  }
  if (total > 0x7FFFFFFF) return VS_ERR_UNSUPPORTED;
  vs_pitch_log2_table(VS_AC_MAX_LAG + 1, (int32_t *)((char *)host + row_bytes));

  VsRecBlock blk;
  rc = vs_rec_upload(ctx, &ctx->rec_pitch, bytes, &blk);
  if (rc != VS_OK) return rc;
  VsPtArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm_dev;
  a.pitch = (long)pitch;
  a.n_lanes = (long)n_lanes;
  a.total_frames = (long)total;
  a.rows = (const VsPtRow *)blk.dev;
  a.lg = (const int32_t *)((const char *)blk.dev + row_bytes);
  a.frames = frames_dev;
  a.frames_pitch = (long)frames_pitch;
  a.voicing_q = o.voicing_q;
  a.octave_q = o.octave_q;
  a.jump_q = o.jump_q;
  a.vuv_q = o.vuv_q;
  a.silence_rms = o.silence_rms;
  return vs_rec_retire(ctx, &blk, vs_launch_pitch(&a, lds, ctx->stream));
}

int vs_pitch(vs_ctx *ctx, const vs_pitch_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
             const int32_t *fs, const int32_t *lengths, size_t frames_pitch, vs_pitch_frame *frames)
{
  const int rc0 = check_args(ctx, pcm, pitch, n_lanes, n_samples, fs, frames_pitch, frames);
  if (rc0 != VS_OK) return rc0;
  /* the PCM in d_in; the records go up and come back, so that what no frame covers comes back as it went */
  VsHostPart parts[1] = {{frames, n_lanes * frames_pitch * sizeof(vs_pitch_frame), VS_PART_UP | VS_PART_DOWN, NULL}};
  int rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 1);
  if (rc != VS_OK) return rc;
  rc = vs_pitch_launch(ctx, opts, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths, frames_pitch,
                       (vs_pitch_frame *)parts[0].dev);
  return vs_host_end(ctx, rc, parts, 1);
}
