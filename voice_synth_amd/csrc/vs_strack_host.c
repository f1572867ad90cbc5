/*
 * vs_strack_host.c -- host side of the source track (include/voice_synth.h, "source track"): the options, the refusals
 * of every lane and row, which cos rows the call can reach, the layout and the contents of the uploaded block (row
 * records, offset table, cos rows), the kernel of vs_strack.hip, the row that plays the pitch track's frames.
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.  The option checks and the row plan
 * touch no device: vs_strack_check, vs_strack_plan and vs_strack_fill are their faces (vs_strack.h).
 */
#include <math.h>
#include <string.h>

#include "vs_strack.h"
#include "vs_internal.h"

int vs_strack_defaults(vs_strack_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->max_reject = 256;
  return VS_OK;
}

int vs_strack_from_pitch(const vs_pitch_opts *pitch_opts, int32_t fs, int32_t len, vs_strack_row *row)
{
  vs_pitch_opts o;
  if (!row) return VS_ERR_ARG;
  if (pitch_opts) o = *pitch_opts;
  else vs_pitch_defaults(&o);
  int32_t n_frames = 0;
  const int rc = vs_pitch_frames(&o, fs, len, &n_frames);
  if (rc != VS_OK) return rc;
  if (n_frames < 1) return VS_ERR_RANGE;
  /* tmin, tmax and H as the header's pitch section has them (vs_pitch_frames has checked their ranges) */
  const int32_t tmin = (int32_t)floor((double)fs / (double)o.f0_max), tmax = (int32_t)ceil((double)fs / (double)o.f0_min);
  const int32_t H = (int32_t)floor(o.hop_s * (double)fs + 0.5);
  row->n_frames = n_frames;
  row->hop = H;
  row->offset = tmax + tmax / 2 - H / 2;
  row->length = len;
  row->pmin = tmin;
  row->pmax = tmax;
  return VS_OK;
}

int vs_strack_check(const vs_strack_opts *opts, size_t n_lanes, size_t n_samples, size_t period_stride,
                    size_t frames_pitch, int has_amp, size_t amp_stride, size_t out_pitch, int has_cycles,
                    size_t cycles_pitch, vs_strack_opts *resolved)
{
  if (n_lanes == 0 || n_samples == 0 || frames_pitch == 0 || out_pitch < n_samples) return VS_ERR_ARG;
  if (period_stride < 4 || (period_stride & 3) != 0) return VS_ERR_ARG;
  if (has_amp && (amp_stride < 4 || (amp_stride & 3) != 0)) return VS_ERR_ARG;
  if (has_cycles && cycles_pitch == 0) return VS_ERR_ARG;
  if (opts) *resolved = *opts;
  else vs_strack_defaults(resolved);
  if (resolved->reserved_ != 0) return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu || out_pitch > 0x7FFFFFFFu ||
      period_stride > 0x7FFFFFFFu || amp_stride > 0x7FFFFFFFu || cycles_pitch > 0x7FFFFFFFu)
    return VS_ERR_UNSUPPORTED;
  if (resolved->max_reject < 1 || resolved->max_reject > VS_ST_MAX_REJECT) return VS_ERR_RANGE;
  return VS_OK;
}

/* T2 = ceil(0.5 * cq * P) (flowgen_shimmer.c:317); monotone in P */
static int t2_of(float cq, int32_t P) { return (int)ceil(0.5 * cq * P); }

int vs_strack_plan(const vs_lane *lanes, const vs_strack_row *rows, size_t n_lanes, size_t n_samples, size_t frames_pitch,
                   uint8_t *need, VsStPlan *plan)
{
  memset(need, 0, VS_ST_T2_MAX + 1);
  int last_a = -1, last_b = -1;
  for (size_t i = 0; i < n_lanes; i++) {
    const int rc = vs_lane_validate(&lanes[i]);
    if (rc != VS_OK) return rc;
    const vs_strack_row *r = &rows[i];
    if (r->n_frames < 1 || (size_t)r->n_frames > frames_pitch || r->hop < 1) return VS_ERR_RANGE;
    if (r->length < 0 || (size_t)r->length > n_samples) return VS_ERR_RANGE;
    if (r->pmin < 2 || r->pmax > VS_AC_MAX_LAG || r->pmin > r->pmax) return VS_ERR_RANGE;
    const int a = t2_of(lanes[i].cq, r->pmin), b = t2_of(lanes[i].cq, r->pmax);
    if (a < 1) return VS_ERR_RANGE;
    if (b > VS_ST_T2_MAX) return VS_ERR_RANGE; /* (cannot happen: cq <= 1) */
    /* (the stretch of the row before is marked already: rows of one command line cost one look) */
    if (a != last_a || b != last_b) memset(need + a, 1, (size_t)(b - a + 1));
    last_a = a;
    last_b = b;
  }
  size_t entries = 0;
  for (int t = 1; t <= VS_ST_T2_MAX; t++)
    if (need[t]) entries += (size_t)t;
  plan->toff_at = n_lanes * sizeof(VsStRow);
  plan->cos_at = plan->toff_at + (((size_t)(VS_ST_T2_MAX + 1) * sizeof(int32_t) + 7) & ~(size_t)7);
  plan->cos_entries = entries;
  plan->bytes = plan->cos_at + entries * sizeof(double);
  return VS_OK;
}

void vs_strack_fill(const vs_lane *lanes, const vs_strack_row *rows, size_t n_lanes, const uint8_t *need,
                    const VsStPlan *plan, void *block)
{
  VsStRow *d = (VsStRow *)block;
  for (size_t i = 0; i < n_lanes; i++) {
    const vs_lane *l = &lanes[i];
    const vs_strack_row *r = &rows[i];
    memset(&d[i], 0, sizeof(d[i]));
    d[i].jitter = l->jitter;
    d[i].shimmer = l->shimmer;
    d[i].K = l->K;
    d[i].Kvar = l->Kvar;
    d[i].DC = l->DC;
    d[i].noise = l->noise;
    d[i].cq = l->cq;
    d[i].amp = l->amp;
    d[i].flags = (((l->flags & VS_FLAG_JITTER) && l->jitter != 0.0) ? VS_STF_JITTER : 0u) |
                 (((l->flags & VS_FLAG_SHIMMER) && l->shimmer != 0.0) ? VS_STF_SHIMMER : 0u) |
                 ((l->flags & VS_FLAG_NOISE) ? VS_STF_NOISE : 0u);
    d[i].key0 = (uint32_t)l->seed;
    d[i].key1 = (uint32_t)(l->seed >> 32);
    d[i].dcs = (int32_t)(int16_t)(int32_t)l->DC;
    d[i].n_frames = r->n_frames;
    d[i].hop = r->hop;
    d[i].offset = r->offset;
    d[i].length = r->length;
    d[i].pmin = r->pmin;
    d[i].pmax = r->pmax;
  }
  int32_t *toff = (int32_t *)((char *)block + plan->toff_at);
  double *cosv = (double *)((char *)block + plan->cos_at);
  memset(toff, 0, plan->cos_at - plan->toff_at);
  size_t at = 0;
  for (int t = 0; t <= VS_ST_T2_MAX; t++) {
    if (!need[t]) {
      toff[t] = -1;
      continue;
    }
    toff[t] = (int32_t)at;
    vs_cos_row(t, cosv + at);
    at += (size_t)t;
  }
}

int vs_strack_launch(vs_ctx *ctx, const vs_strack_opts *opts, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                     const vs_strack_row *rows, const int32_t *period_dev, size_t period_stride, size_t frames_pitch,
                     const int32_t *amp_dev, size_t amp_stride, int16_t *flow_dev, size_t out_pitch,
                     vs_strack_stat *stat_dev, vs_strack_cycle *cycles_dev, size_t cycles_pitch)
{
  vs_strack_opts o;
  uint8_t need[VS_ST_T2_MAX + 1];
  VsStPlan plan;
  if (!ctx || !lanes || !rows || !period_dev || !flow_dev || !stat_dev) return VS_ERR_ARG;
  if (((uintptr_t)period_dev & 3) != 0 || ((uintptr_t)amp_dev & 3) != 0) return VS_ERR_ARG;
  int rc = vs_strack_check(opts, n_lanes, n_samples, period_stride, frames_pitch, amp_dev != NULL, amp_stride, out_pitch,
                           cycles_dev != NULL, cycles_pitch, &o);
  if (rc != VS_OK) return rc;
  rc = vs_strack_plan(lanes, rows, n_lanes, n_samples, frames_pitch, need, &plan);
  if (rc != VS_OK) return rc;
  if (plan.cos_entries > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED; /* (cannot happen: at most 1025 rows of at most 1025) */

  void *host = NULL;
  VsRecBlock blk;
  rc = vs_rec_stage(ctx, &ctx->rec_strack, plan.bytes, &host);
  if (rc != VS_OK) return rc;
  vs_strack_fill(lanes, rows, n_lanes, need, &plan, host);
  rc = vs_rec_upload(ctx, &ctx->rec_strack, plan.bytes, &blk);
  if (rc != VS_OK) return rc;
  VsStArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = (const VsStRow *)blk.dev;
  a.toff = (const int32_t *)((const char *)blk.dev + plan.toff_at);
  a.costab = (const double *)((const char *)blk.dev + plan.cos_at);
  a.period = (const char *)period_dev;
  a.amp = (const char *)amp_dev;
  a.period_stride = (int)period_stride;
  a.amp_stride = amp_dev ? (int)amp_stride : 0;
  a.frames_pitch = (long)frames_pitch;
  a.out = flow_dev;
  a.out_pitch = (long)out_pitch;
  a.stat = stat_dev;
  a.cycles = cycles_dev;
  a.cycles_pitch = cycles_dev ? (int)cycles_pitch : 0;
  a.n_lanes = (long)n_lanes;
  a.max_reject = o.max_reject;
  return vs_rec_retire(ctx, &blk, vs_launch_strack(&a, ctx->stream));
}

int vs_strack(vs_ctx *ctx, const vs_strack_opts *opts, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
              const vs_strack_row *rows, const int32_t *period, size_t frames_pitch, const int32_t *amp, int16_t *flow,
              vs_strack_stat *stat, vs_strack_cycle *cycles, size_t cycles_pitch)
{
  vs_strack_opts o;
  uint8_t need[VS_ST_T2_MAX + 1];
  VsStPlan plan;
  if (!ctx || !lanes || !rows || !period || !flow || !stat) return VS_ERR_ARG;
  int rc = vs_strack_check(opts, n_lanes, n_samples, 4, frames_pitch, amp != NULL, 4, n_samples, cycles != NULL,
                           cycles_pitch, &o);
  if (rc != VS_OK) return rc;
  rc = vs_strack_plan(lanes, rows, n_lanes, n_samples, frames_pitch, need, &plan); /* refused before anything moves */
  if (rc != VS_OK) return rc;
  /* the periods in d_in; the amplitudes go up; the flow goes up and comes back (what lies past a row's length comes back
   * as it went), the cycle records too; the status records come back */
  const size_t track_bytes = n_lanes * frames_pitch * sizeof(int32_t);
  VsHostPart parts[4] = {{(void *)amp, track_bytes, VS_PART_UP, NULL},
                         {flow, n_lanes * n_samples * sizeof(int16_t), VS_PART_UP | VS_PART_DOWN, NULL},
                         {stat, n_lanes * sizeof(vs_strack_stat), VS_PART_DOWN, NULL},
                         {cycles, n_lanes * cycles_pitch * sizeof(vs_strack_cycle), VS_PART_UP | VS_PART_DOWN, NULL}};
  rc = vs_host_begin(ctx, period, track_bytes, parts, 4);
  if (rc != VS_OK) return rc;
  rc = vs_strack_launch(ctx, &o, lanes, n_lanes, n_samples, rows, (const int32_t *)ctx->pool.d_in, 4, frames_pitch,
                        (const int32_t *)parts[0].dev, 4, (int16_t *)parts[1].dev, n_samples,
                        (vs_strack_stat *)parts[2].dev, (vs_strack_cycle *)parts[3].dev, cycles_pitch);
  return vs_host_end(ctx, rc, parts, 4);
}
