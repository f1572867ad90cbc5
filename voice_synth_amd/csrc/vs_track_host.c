/*
 * vs_track_host.c -- host side of the coefficient tracks (include/voice_synth.h, "coefficient tracks"): validation, the
 * upload of the per-row records, the kernels of vs_track.hip, and the host-only helpers (step-down, step-up, the sets of
 * a glide, the row that plays vs_lpc's frames).
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.
 */
#include <math.h>
#include <string.h>

#include "vs_track.h"
#include "vs_internal.h"

/* the header's step-down: k[0..p) = k_1..k_p of A[1..p]; 0, or -1 for a tap that is not finite or a |k_i| >= 1 */
static int step_down(int p, const double *A, double *k)
{
  double a[VS_MAX_NCOEF], na[VS_MAX_NCOEF];
  for (int j = 1; j <= p; j++) {
    if (!isfinite(A[j])) return -1;
    a[j] = A[j];
  }
  for (int i = p; i >= 1; i--) {
    const double ki = a[i];
    if (!(fabs(ki) < 1.0)) return -1;
    k[i - 1] = ki;
    const double d = 1.0 - ki * ki;
    for (int j = 1; j < i; j++) na[j] = (a[j] - ki * a[i - j]) / d;
    for (int j = 1; j < i; j++) a[j] = na[j];
  }
  return 0;
}

/* the header's step-up: A[0] = 1, A[1..p] from kappa[0..p) */
static void step_up(int p, const double *kappa, double *A)
{
  double a[VS_MAX_NCOEF], na[VS_MAX_NCOEF];
  for (int i = 1; i <= p; i++) {
    const double ki = kappa[i - 1];
    for (int j = 1; j < i; j++) na[j] = a[j] + ki * a[i - j];
    for (int j = 1; j < i; j++) a[j] = na[j];
    a[i] = ki;
  }
  A[0] = 1.0;
  for (int j = 1; j <= p; j++) A[j] = a[j];
}

int vs_track_reflection(int order, const double *A, double *k)
{
  if (!A || !k) return VS_ERR_ARG;
  if (order < 1 || order > VS_MAX_ORDER) return VS_ERR_RANGE;
  return step_down(order, A, k) == 0 ? VS_OK : VS_ERR_RANGE;
}

int vs_track_glide_sets(int order, const double *A_from, const double *A_to, int n_sets, double *coefs)
{
  if (!A_from || !A_to || !coefs) return VS_ERR_ARG;
  if (order < 1 || order > VS_MAX_ORDER || n_sets < 2) return VS_ERR_RANGE;
  double kf[VS_MAX_ORDER], kt[VS_MAX_ORDER], kap[VS_MAX_ORDER];
  if (step_down(order, A_from, kf) != 0 || step_down(order, A_to, kt) != 0) return VS_ERR_RANGE;
  for (int s = 0; s < n_sets; s++) {
    const double t = (double)s / (double)(n_sets - 1);
    for (int i = 0; i < order; i++) kap[i] = kf[i] + t * (kt[i] - kf[i]);
    step_up(order, kap, coefs + (size_t)s * (size_t)(order + 1));
  }
  return VS_OK;
}

int vs_track_from_lpc(const vs_lpc_opts *opts, int32_t fs, int32_t len, int mode, vs_track_row *row)
{
  vs_lpc_opts o;
  if (!row || (mode != VS_TRACK_HOLD && mode != VS_TRACK_GLIDE)) return VS_ERR_ARG;
  if (opts) o = *opts;
  else vs_lpc_defaults(&o);
  int32_t n_frames = 0;
  const int rc = vs_lpc_frames(&o, fs, len, &n_frames);
  if (rc != VS_OK) return rc;
  if (n_frames < 1 || !(o.hop_s > 0.0)) return VS_ERR_RANGE;
  /* L, H and s0 as the header's LPC section has them (vs_lpc_frames has checked their ranges) */
  const int32_t L = (int32_t)floor(o.window_s * (double)fs + 0.5), H = (int32_t)floor(o.hop_s * (double)fs + 0.5);
  const int32_t s0 = o.pre_emphasis;
  row->n_sets = n_frames;
  row->hop = H;
  row->offset = mode == VS_TRACK_GLIDE ? s0 + L / 2 : s0 + L / 2 - H / 2;
  row->length = len;
  row->gain = 1.0f;
  row->pre_emphasis = 0.0f;
  return VS_OK;
}

int vs_setwalk_check(int mode, int order, size_t in_pitch, size_t out_pitch, size_t n_lanes, size_t n_samples,
                     size_t sets_pitch, const int32_t *n_sets, const int32_t *hop, const int32_t *length,
                     size_t row_bytes)
{
  if (n_lanes == 0 || n_samples == 0 || sets_pitch == 0 || in_pitch < n_samples || out_pitch < n_samples)
    return VS_ERR_ARG;
  if (mode != VS_TRACK_HOLD && mode != VS_TRACK_GLIDE) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || sets_pitch > 0x7FFFFFFFu || in_pitch > 0x7FFFFFFFu ||
      out_pitch > 0x7FFFFFFFu)
    return VS_ERR_UNSUPPORTED;
  if (order < 1 || order > VS_MAX_ORDER) return VS_ERR_RANGE;
  for (size_t i = 0; i < n_lanes; i++) {
    const size_t at = i * row_bytes;
    const int32_t ns = *(const int32_t *)((const char *)n_sets + at), h = *(const int32_t *)((const char *)hop + at),
                  len = *(const int32_t *)((const char *)length + at);
    if (ns < 1 || (size_t)ns > sets_pitch || h < 1 || len < 0 || (size_t)len > n_samples) return VS_ERR_RANGE;
  }
  return VS_OK;
}
/* ... of vs_track_row records */
static int check_call(int mode, int order, size_t in_pitch, size_t out_pitch, size_t n_lanes, size_t n_samples,
                      const vs_track_row *rows, size_t sets_pitch)
{
  return vs_setwalk_check(mode, order, in_pitch, out_pitch, n_lanes, n_samples, sets_pitch, &rows->n_sets, &rows->hop,
                          &rows->length, sizeof(*rows));
}

int vs_track_launch(vs_ctx *ctx, int mode, int order, const int16_t *flow_dev, size_t in_pitch, int16_t *out_dev,
                    size_t out_pitch, size_t n_lanes, size_t n_samples, const vs_track_row *rows,
                    const double *coefs_dev, const double *gains_dev, size_t sets_pitch, vs_track_stat *stat_dev)
{
  if (!ctx || !flow_dev || !out_dev || !rows || !coefs_dev) return VS_ERR_ARG;
  int rc = check_call(mode, order, in_pitch, out_pitch, n_lanes, n_samples, rows, sets_pitch);
  if (rc != VS_OK) return rc;

  const size_t bytes = n_lanes * sizeof(vs_track_row);
  void *host = NULL;
  VsRecBlock blk;
  rc = vs_rec_stage(ctx, &ctx->rec_track, bytes, &host);
  if (rc != VS_OK) return rc;
  memcpy(host, rows, bytes);
  rc = vs_rec_upload(ctx, &ctx->rec_track, bytes, &blk);
  if (rc != VS_OK) return rc;
  VsTrackArgs a;
  memset(&a, 0, sizeof(a));
  a.in = flow_dev;
  a.out = out_dev;
  a.in_pitch = (long)in_pitch;
  a.out_pitch = (long)out_pitch;
  a.n_lanes = (long)n_lanes;
  a.rows = (const vs_track_row *)blk.dev;
  a.coefs = coefs_dev;
  a.gains = gains_dev;
  a.stat = stat_dev;
  a.sets_pitch = (long)sets_pitch;
  a.order = order;
  a.vec_ok = vs_vec_ok(flow_dev, in_pitch, out_dev, out_pitch);
  return vs_rec_retire(ctx, &blk, vs_launch_track(ctx->arith, mode, &a, ctx->stream));
}

int vs_track(vs_ctx *ctx, int mode, int order, const int16_t *flow, int16_t *pcm, size_t n_lanes, size_t n_samples,
             const vs_track_row *rows, const double *coefs, const double *gains, size_t sets_pitch, vs_track_stat *stat)
{
  if (!ctx || !flow || !pcm || !rows || !coefs) return VS_ERR_ARG;
  int rc = check_call(mode, order, n_samples, n_samples, n_lanes, n_samples, rows, sets_pitch);
  if (rc != VS_OK) return rc;
  /* the flow in d_in; the PCM goes up and comes back (what lies past a row's length comes back as it went), the sets
   * and the gains go up, the status records come back */
  const size_t pcm_bytes = n_lanes * n_samples * sizeof(int16_t), n_sets = n_lanes * sets_pitch;
  VsHostPart parts[4] = {{pcm, pcm_bytes, VS_PART_UP | VS_PART_DOWN, NULL},
                         {(void *)coefs, n_sets * (size_t)(order + 1) * sizeof(double), VS_PART_UP, NULL},
                         {(void *)gains, n_sets * sizeof(double), VS_PART_UP, NULL},
                         {stat, n_lanes * sizeof(vs_track_stat), VS_PART_DOWN, NULL}};
  rc = vs_host_begin(ctx, flow, pcm_bytes, parts, 4);
  if (rc != VS_OK) return rc;
  rc = vs_track_launch(ctx, mode, order, (const int16_t *)ctx->pool.d_in, n_samples, (int16_t *)parts[0].dev, n_samples,
                       n_lanes, n_samples, rows, (const double *)parts[1].dev, (const double *)parts[2].dev, sets_pitch,
                       (vs_track_stat *)parts[3].dev);
  return vs_host_end(ctx, rc, parts, 4);
}
