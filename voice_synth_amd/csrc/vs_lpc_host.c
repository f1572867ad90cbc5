/*
 * vs_lpc_host.c -- host side of the LPC analysis (include/voice_synth.h, "LPC analysis"): the options, the frames of
 * every row, the window tables, the upload of the per-row records, the kernel of vs_lpc.hip.
 * Plain C against the HIP runtime's C API, like the rest of the library's host side.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "vs_lpc.h"
#include "vs_internal.h"

int vs_lpc_defaults(vs_lpc_opts *opts)
{
  if (!opts) return VS_ERR_ARG;
  memset(opts, 0, sizeof(*opts));
  opts->order = VS_ORDER;
  opts->window = VS_LPC_HAMMING;
  opts->pre_emphasis = 0;
  opts->n_formants = 5;
  opts->window_s = 0.025;
  opts->hop_s = 0.010;
  opts->f_lo = 50.0;
  return VS_OK;
}

static int check_opts(const vs_lpc_opts *o)
{
  if (o->window != VS_LPC_HAMMING && o->window != VS_LPC_RECTANGULAR) return VS_ERR_ARG;
  if ((o->pre_emphasis != 0 && o->pre_emphasis != 1) || o->reserved_ != 0) return VS_ERR_ARG;
  if (o->n_formants < 0 || o->n_formants > VS_LPC_MAX_FORMANTS) return VS_ERR_ARG;
  if (!isfinite(o->window_s) || !isfinite(o->hop_s) || !isfinite(o->f_lo) || !(o->hop_s >= 0.0) || !(o->f_lo >= 0.0))
    return VS_ERR_ARG;
  if (o->order < 1 || o->order > VS_MAX_ORDER) return VS_ERR_RANGE;
  return VS_OK;
}

/* L, H, the start of frame 0 and the frame count of one row (the header's formulas); VS_ERR_RANGE outside the limits */
static int row_frames(const vs_lpc_opts *o, int32_t fs, int32_t len, VsLpcRow *r)
{
  if (fs <= 0 || len < 0) return VS_ERR_RANGE;
  const double Ld = floor(o->window_s * (double)fs + 0.5), Hd = floor(o->hop_s * (double)fs + 0.5);
  if (!(Ld > (double)o->order) || !(Ld <= (double)VS_LPC_MAX_WINDOW)) return VS_ERR_RANGE;
  const int32_t L = (int32_t)Ld, pre = o->pre_emphasis;
  r->fs = fs;
  r->L = L;
  r->H = 0;
  r->s0 = pre;
  r->n_frames = 0;
  if (o->hop_s > 0.0) {
    if (!(Hd >= 1.0) || Hd > 2147483647.0) return VS_ERR_RANGE;
    r->H = (int32_t)Hd;
    if ((int64_t)len >= (int64_t)pre + L) r->n_frames = 1 + (len - pre - L) / r->H;
  } else if ((int64_t)len >= (int64_t)pre + L) {
    r->s0 = pre + (len - pre - L) / 2;
    r->n_frames = 1;
  }
  return VS_OK;
}

/* ... and the one frame over the whole row that the closed-phase analysis takes with window_s == 0 */
int vs_lpc_row_whole(int32_t fs, int32_t len, VsLpcRow *r)
{
  if (fs <= 0 || len < 0) return VS_ERR_RANGE;
  memset(r, 0, sizeof(*r));
  r->fs = fs;
  r->L = len;
  r->n_frames = 1;
  return VS_OK;
}

int vs_lpc_frames(const vs_lpc_opts *opts, int32_t fs, int32_t len, int32_t *n_frames)
{
  vs_lpc_opts o;
  if (!n_frames) return VS_ERR_ARG;
  VS_OPTS_OR(o, opts, vs_lpc_defaults);
  int rc = check_opts(&o);
  if (rc != VS_OK) return rc;
  VsLpcRow r;
  rc = row_frames(&o, fs, len, &r);
  if (rc != VS_OK) return rc;
  *n_frames = r.n_frames;
  return VS_OK;
}

int vs_lpc_window(int32_t L, int32_t window, int32_t *w)
{
  if (!w) return VS_ERR_ARG;
  if (window != VS_LPC_HAMMING && window != VS_LPC_RECTANGULAR) return VS_ERR_ARG;
  if (L < 2 || L > VS_LPC_MAX_WINDOW) return VS_ERR_RANGE;
  const double pi = 3.14159265358979323846;
  for (int32_t n = 0; n < L; n++)
    w[n] = window == VS_LPC_RECTANGULAR ? 256
                                        : (int32_t)floor(256.0 * (0.54 - 0.46 * cos(2.0 * pi * (double)n / (double)(L - 1))) + 0.5);
  return VS_OK;
}

static int cmp_i32(const void *x, const void *y)
{
  const int32_t a = *(const int32_t *)x, b = *(const int32_t *)y;
  return (a > b) - (a < b);
}

int vs_lpc_check_opts(const vs_lpc_opts *o) { return check_opts(o); }

int vs_frame_check(const vs_ctx *ctx, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
                   const int32_t *fs, size_t frames_pitch, const vs_lpc_frame *frames, int need_frames_pitch)
{
  if (!ctx || !pcm || !fs || !frames || n_lanes == 0 || n_samples == 0 || pitch < n_samples ||
      (need_frames_pitch && frames_pitch == 0))
    return VS_ERR_ARG;
  if (n_lanes > 0x7FFFFFFFu || n_samples > 0x7FFFFFFFu || frames_pitch > 0x7FFFFFFFu) return VS_ERR_UNSUPPORTED;
  return VS_OK;
}

void vs_frame_parts(VsHostPart *parts, size_t nfr, int order, int n_formants, vs_lpc_frame *frames, double *formants,
                    double *coefs)
{
  const unsigned both = VS_PART_UP | VS_PART_DOWN;
  parts[0] = (VsHostPart){frames, nfr * sizeof(vs_lpc_frame), both, NULL};
  parts[1] = (VsHostPart){formants, nfr * 2 * (size_t)n_formants * sizeof(double), both, NULL};
  parts[2] = (VsHostPart){coefs, nfr * (size_t)(order + 1) * sizeof(double), both, NULL};
}

int vs_lpc_rows_upload(vs_ctx *ctx, VsRecSlot *slot, const vs_lpc_opts *opts, int whole, const int16_t *pcm_dev,
                       size_t pitch, size_t n_lanes, size_t n_samples, const int32_t *fs, const int32_t *lengths,
                       size_t frames_pitch, vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev,
                       VsRecBlock *blk_out, VsLpcArgs *args)
{
  const vs_lpc_opts o = *opts;
  int rc = vs_frame_check(ctx, pcm_dev, pitch, n_lanes, n_samples, fs, frames_pitch, frames_dev, 0);
  if (rc == VS_OK) rc = check_opts(&o);
  if (rc != VS_OK) return rc;

  /* every row's frames, and the distinct window lengths (sorted) before anything touches the device */
  VsLpcRow *rows_tmp = (VsLpcRow *)malloc(n_lanes * sizeof(VsLpcRow));
  /* one allocation, two arrays of n_lanes: Ls, first every row's L, then the nL distinct ones; woff, the second half,
   * indexed like the distinct Ls: woff[k] = where the table of Ls[k] starts.  (The compaction below writes Ls[nL] at or
   * before the element it reads, and never reaches woff.) */
  int32_t *Ls = (int32_t *)malloc(2 * n_lanes * sizeof(int32_t));
  int32_t *woff = Ls ? Ls + n_lanes : NULL;
  if (!rows_tmp || !Ls) rc = VS_ERR_NOMEM;
  int64_t total = 0;
  for (size_t i = 0; i < n_lanes && rc == VS_OK; i++) {
    const int32_t len = lengths ? lengths[i] : (int32_t)n_samples;
    if (len < 0 || (size_t)len > n_samples) rc = VS_ERR_ARG;
    else rc = whole ? vs_lpc_row_whole(fs[i], len, &rows_tmp[i]) : row_frames(&o, fs[i], len, &rows_tmp[i]);
    if (rc == VS_OK && (size_t)rows_tmp[i].n_frames > frames_pitch) rc = VS_ERR_RANGE;
    if (rc == VS_OK) {
      rows_tmp[i].first = total;
      total += rows_tmp[i].n_frames;
      Ls[i] = rows_tmp[i].L;
    }
  }
  size_t nL = 0, wtotal = 0; /* whole rows have no window: no table */
  if (rc == VS_OK && !whole) {
    qsort(Ls, n_lanes, sizeof(int32_t), cmp_i32);
    for (size_t i = 0; i < n_lanes; i++)
      if (i == 0 || Ls[i] != Ls[i - 1]) {
        woff[nL] = (int32_t)wtotal;
        Ls[nL++] = Ls[i];
        wtotal += (size_t)Ls[i];
      }
  }
  const size_t row_bytes = n_lanes * sizeof(VsLpcRow), bytes = row_bytes + wtotal * sizeof(int32_t);
  void *host = NULL;
  if (rc == VS_OK) rc = vs_rec_stage(ctx, slot, bytes, &host);
  if (rc == VS_OK) {
    /* [rows][window tables, one per distinct L in ascending L] */
    VsLpcRow *rows = (VsLpcRow *)host;
    int32_t *win = (int32_t *)((char *)host + row_bytes);
    for (size_t k = 0; k < nL; k++) vs_lpc_window(Ls[k], o.window, win + woff[k]);
    for (size_t i = 0; i < n_lanes && nL > 0; i++) {
      size_t lo = 0, hi = nL - 1; /* Ls[lo] == rows_tmp[i].L */
      while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (Ls[mid] < rows_tmp[i].L) lo = mid + 1;
        else hi = mid;
      }
      rows_tmp[i].woff = woff[lo];
    }
    memcpy(rows, rows_tmp, row_bytes);
  }
  free(rows_tmp);
  free(Ls);
  if (rc != VS_OK) return rc;

  VsRecBlock blk;
  rc = vs_rec_upload(ctx, slot, bytes, &blk);
  if (rc != VS_OK) return rc;
  VsLpcArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm_dev;
  a.pitch = (long)pitch;
  a.n_lanes = (long)n_lanes;
  a.total_frames = (long)total;
  a.rows = (const VsLpcRow *)blk.dev;
  a.windows = whole ? NULL : (const int32_t *)((char *)blk.dev + row_bytes);
  a.frames = frames_dev;
  a.formants = formants_dev;
  a.coefs = coefs_dev;
  a.frames_pitch = (long)frames_pitch;
  a.order = o.order;
  a.pre = o.pre_emphasis;
  a.n_formants = o.n_formants;
  a.f_lo = o.f_lo;
  *args = a;
  *blk_out = blk;
  return VS_OK;
}

int vs_lpc_launch(vs_ctx *ctx, const vs_lpc_opts *opts, const int16_t *pcm_dev, size_t pitch, size_t n_lanes,
                  size_t n_samples, const int32_t *fs, const int32_t *lengths, size_t frames_pitch,
                  vs_lpc_frame *frames_dev, double *formants_dev, double *coefs_dev)
{
  vs_lpc_opts o;
  if (!ctx) return VS_ERR_ARG;
  VS_OPTS_OR(o, opts, vs_lpc_defaults);
  VsRecBlock blk;
  VsLpcArgs a;
  const int rc = vs_lpc_rows_upload(ctx, &ctx->rec_lpc, &o, 0, pcm_dev, pitch, n_lanes, n_samples, fs, lengths,
                                    frames_pitch, frames_dev, formants_dev, coefs_dev, &blk, &a);
  if (rc != VS_OK) return rc;
  return vs_rec_retire(ctx, &blk, vs_launch_lpc(&a, ctx->stream));
}

int vs_lpc(vs_ctx *ctx, const vs_lpc_opts *opts, const int16_t *pcm, size_t pitch, size_t n_lanes, size_t n_samples,
           const int32_t *fs, const int32_t *lengths, size_t frames_pitch, vs_lpc_frame *frames, double *formants,
           double *coefs)
{
  vs_lpc_opts o;
  int rc = vs_frame_check(ctx, pcm, pitch, n_lanes, n_samples, fs, frames_pitch, frames, 1);
  if (rc != VS_OK) return rc;
  VS_OPTS_OR(o, opts, vs_lpc_defaults);
  rc = check_opts(&o);
  if (rc != VS_OK) return rc;
  /* the PCM in d_in; the records, the formants and the coefficients go up and come back */
  VsHostPart parts[3];
  vs_frame_parts(parts, n_lanes * frames_pitch, o.order, o.n_formants, frames, formants, coefs);
  rc = vs_host_begin(ctx, pcm, ((n_lanes - 1) * pitch + n_samples) * sizeof(int16_t), parts, 3);
  if (rc != VS_OK) return rc;
  rc = vs_lpc_launch(ctx, &o, (const int16_t *)ctx->pool.d_in, pitch, n_lanes, n_samples, fs, lengths, frames_pitch,
                     (vs_lpc_frame *)parts[0].dev, (double *)parts[1].dev, (double *)parts[2].dev);
  return vs_host_end(ctx, rc, parts, 3);
}
