/*
 * test_cplpc_host_asan.c -- the device-free half of the closed-phase covariance LPC (csrc/vs_cplpc_host.c, on top of
 * csrc/vs_lpc_host.c) under AddressSanitizer + UndefinedBehaviorSanitizer: the defaults, every refusal of the options,
 * vs_cplpc_frames and vs_cplpc_lpc_opts against vs_lpc_frames, and -- with stand-ins for the record upload, the
 * host-buffer call and the launcher, which only keep what they are handed -- the arguments vs_cplpc_launch and vs_cplpc
 * refuse and the row records and launch arguments they build.  Needs the HIP runtime's C header only.  Prints "ok".
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../voice_synth_amd/csrc/vs_cplpc.h"
#include "../../voice_synth_amd/csrc/vs_internal.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      exit(1);                                                     \
    }                                                              \
  } while (0)

/* ---- stand-ins: the record upload keeps the staged bytes in a block of exactly that size, the launcher copies the
 * arguments and the rows it was given, the host-buffer call hands the caller's arrays through ---- */
static void *staged;
static size_t staged_bytes;
static VsCplpcArgs seen;
static VsLpcRow seen_rows[64];
static size_t seen_bytes; /* of the staged block the launch read its rows from */
static int32_t seen_win[4096]; /* ... and what lies behind the rows in it */
static int launches, lpc_launches;

int vs_rec_stage(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, void **host)
{
  CHECK(slot == &ctx->rec_cplpc && !staged);
  staged = malloc(bytes ? bytes : 1);
  staged_bytes = bytes;
  *host = staged;
  return VS_OK;
}
int vs_rec_upload(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, VsRecBlock *blk)
{
  CHECK(staged && bytes == staged_bytes);
  blk->dev = staged;
  blk->cap = bytes;
  return VS_OK;
}
int vs_rec_retire(vs_ctx *ctx, VsRecBlock *blk, hipError_t launched)
{
  CHECK(blk->dev == staged);
  free(staged);
  staged = NULL;
  return launched == hipSuccess ? VS_OK : VS_ERR_HIP;
}
hipError_t vs_launch_cplpc(const VsCplpcArgs *a, hipStream_t s)
{
  seen = *a;
  CHECK(a->lpc.n_lanes <= 64 && (size_t)a->lpc.n_lanes * sizeof(VsLpcRow) <= staged_bytes);
  memcpy(seen_rows, a->lpc.rows, (size_t)a->lpc.n_lanes * sizeof(VsLpcRow));
  seen_bytes = staged_bytes;
  const size_t behind = staged_bytes - (size_t)a->lpc.n_lanes * sizeof(VsLpcRow);
  CHECK((const void *)a->lpc.rows == staged && behind <= sizeof(seen_win));
  memcpy(seen_win, (const char *)staged + staged_bytes - behind, behind);
  launches++;
  return hipSuccess;
}
hipError_t vs_launch_lpc(const VsLpcArgs *a, hipStream_t s)
{
  lpc_launches++;
  return hipSuccess;
}
int vs_host_begin(vs_ctx *ctx, const void *in, size_t in_bytes, VsHostPart *parts, int n_parts)
{
  ctx->pool.d_in = (void *)in;
  for (int k = 0; k < n_parts; k++) parts[k].dev = parts[k].host && parts[k].bytes ? parts[k].host : NULL;
  return VS_OK;
}
int vs_host_end(vs_ctx *ctx, int launch_rc, const VsHostPart *parts, int n_parts) { return launch_rc; }

static int opts_rc(const vs_cplpc_opts *o)
{
  vs_lpc_opts lo;
  int32_t n = -7;
  const int a = vs_cplpc_lpc_opts(o, &lo), b = vs_cplpc_frames(o, 16000, 16000, &n);
  CHECK(b == a || (a == VS_OK && b == VS_ERR_RANGE)); /* (a window no frame fits is the row's refusal) */
  return a;
}

int main(void)
{
  vs_cplpc_opts d, o;
  vs_lpc_opts lo;
  int32_t n = 0, m = 0;
  CHECK(sizeof(vs_cplpc_opts) == 56);
  CHECK(vs_cplpc_defaults(NULL) == VS_ERR_ARG && vs_cplpc_defaults(&d) == VS_OK);
  CHECK(d.order == VS_ORDER && d.anchor == VS_CP_ANCHOR_CLOSE && d.delay == 4 && d.span_q == 77 && d.min_equations == 0);
  CHECK(d.n_formants == 5 && d.window_s == 0.0 && d.hop_s == 0.010 && d.f_lo == 50.0 && d.reserved_ == 0);
  CHECK((VS_CP_FEW_EQUATIONS | VS_CP_SINGULAR | VS_CP_NOT_MINIMUM_PHASE) == 0x70);
  CHECK(((VS_CP_FEW_EQUATIONS | VS_CP_SINGULAR | VS_CP_NOT_MINIMUM_PHASE) & (VS_LPC_SILENT | VS_LPC_UNSTABLE | VS_LPC_NO_ROOTS)) == 0);
  CHECK(vs_cplpc_lpc_opts(&d, NULL) == VS_ERR_ARG && vs_cplpc_frames(&d, 16000, 100, NULL) == VS_ERR_ARG);
  CHECK(vs_cplpc_lpc_opts(NULL, &lo) == VS_OK && lo.order == VS_ORDER && lo.pre_emphasis == 0 && lo.window_s == 0.0);

  /* the ranges, each at its last good and its first bad value */
#define WITH(field, value) (o = d, o.field = (value), opts_rc(&o))
  CHECK(opts_rc(&d) == VS_OK);
  CHECK(WITH(order, 1) == VS_OK && WITH(order, VS_MAX_ORDER) == VS_OK);
  CHECK(WITH(order, 0) == VS_ERR_RANGE && WITH(order, VS_MAX_ORDER + 1) == VS_ERR_RANGE && WITH(order, -2147483647 - 1) == VS_ERR_RANGE);
  CHECK(WITH(anchor, VS_CP_ANCHOR_PEAK) == VS_OK && WITH(anchor, 3) == VS_ERR_RANGE && WITH(anchor, -1) == VS_ERR_RANGE);
  CHECK(WITH(delay, -32768) == VS_OK && WITH(delay, 32767) == VS_OK);
  CHECK(WITH(delay, -32769) == VS_ERR_RANGE && WITH(delay, 32768) == VS_ERR_RANGE && WITH(delay, 2147483647) == VS_ERR_RANGE);
  CHECK(WITH(span_q, 1) == VS_OK && WITH(span_q, 256) == VS_OK && WITH(span_q, 0) == VS_ERR_RANGE && WITH(span_q, 257) == VS_ERR_RANGE);
  CHECK(WITH(min_equations, VS_ORDER) == VS_OK && WITH(min_equations, 2147483647) == VS_OK);
  CHECK(WITH(min_equations, VS_ORDER - 1) == VS_ERR_RANGE && WITH(min_equations, -1) == VS_ERR_RANGE);
  CHECK(WITH(n_formants, 0) == VS_OK && WITH(n_formants, VS_LPC_MAX_FORMANTS) == VS_OK);
  CHECK(WITH(n_formants, -1) == VS_ERR_ARG && WITH(n_formants, VS_LPC_MAX_FORMANTS + 1) == VS_ERR_ARG);
  CHECK(WITH(reserved_, 1) == VS_ERR_ARG && WITH(f_lo, -1.0) == VS_ERR_ARG && WITH(f_lo, NAN) == VS_ERR_ARG);
  CHECK(WITH(hop_s, -0.01) == VS_ERR_ARG && WITH(hop_s, INFINITY) == VS_ERR_ARG && WITH(window_s, NAN) == VS_ERR_ARG);
  CHECK(WITH(window_s, -0.01) == VS_ERR_RANGE && WITH(window_s, 0.025) == VS_OK);

  /* frames: one per row with window_s == 0, whatever the length; else vs_lpc_frames of the options vs_cplpc_lpc_opts gives */
  CHECK(vs_cplpc_frames(&d, 16000, 0, &n) == VS_OK && n == 1 && vs_cplpc_frames(&d, 16000, 2147483647, &n) == VS_OK && n == 1);
  CHECK(vs_cplpc_frames(&d, 0, 100, &n) == VS_ERR_RANGE && vs_cplpc_frames(&d, 16000, -1, &n) == VS_ERR_RANGE);
  o = d;
  o.window_s = 0.05;
  o.hop_s = 0.025;
  CHECK(vs_cplpc_lpc_opts(&o, &lo) == VS_OK && lo.window_s == 0.05 && lo.hop_s == 0.025 && lo.order == o.order && lo.pre_emphasis == 0);
  const int32_t lens[] = {0, 1, 799, 800, 801, 1199, 1200, 16000, 2147483647};
  for (size_t k = 0; k < sizeof(lens) / sizeof(lens[0]); k++) {
    CHECK(vs_cplpc_frames(&o, 16000, lens[k], &n) == VS_OK && vs_lpc_frames(&lo, 16000, lens[k], &m) == VS_OK && n == m);
    CHECK(n == (lens[k] >= 800 ? 1 + (lens[k] - 800) / 400 : 0));
  }
  o.window_s = 0.0001; /* L = 2 <= order */
  CHECK(vs_cplpc_frames(&o, 16000, 16000, &n) == VS_ERR_RANGE);
  o.window_s = 2.0;    /* L beyond VS_LPC_MAX_WINDOW */
  CHECK(vs_cplpc_frames(&o, 16000, 16000, &n) == VS_ERR_RANGE);

  /* the launch: refusals before anything is staged, then the rows and arguments it builds */
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(struct vs_ctx));
  CHECK(ctx);
  enum { ROWS = 5, NS = 4000, PITCH = 4008, CP = 7, FP = 20 };
  int16_t *pcm = (int16_t *)calloc((size_t)ROWS * PITCH, sizeof(int16_t));
  vs_glottal_rec *gl = (vs_glottal_rec *)calloc(ROWS, sizeof(vs_glottal_rec));
  vs_glottal_cycle *cy = (vs_glottal_cycle *)calloc((size_t)ROWS * CP, sizeof(vs_glottal_cycle));
  vs_lpc_frame *fr = (vs_lpc_frame *)calloc((size_t)ROWS * FP, sizeof(vs_lpc_frame));
  double *cf = (double *)calloc((size_t)ROWS * FP * (VS_MAX_ORDER + 1), sizeof(double));
  int32_t *cnt = (int32_t *)calloc((size_t)ROWS * FP * 2, sizeof(int32_t));
  CHECK(pcm && gl && cy && fr && cf && cnt);
  int32_t fs[ROWS] = {16000, 16000, 8000, 16000, 22050}, len[ROWS] = {4000, 0, 3999, 17, 2500};
#define LAUNCH(o_, pcm_, pitch_, rows_, ns_, fs_, len_, gl_, cy_, cp_, fp_, fr_) \
  vs_cplpc_launch(ctx, o_, pcm_, pitch_, rows_, ns_, fs_, len_, gl_, cy_, cp_, fp_, fr_, NULL, cf, cnt)
  CHECK(vs_cplpc_launch(NULL, &d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, fr, NULL, cf, cnt) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, NULL, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, NULL, len, gl, cy, CP, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, NULL, cy, CP, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, NULL, CP, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, NULL) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, 0, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, 0, fs, len, gl, cy, CP, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, NS - 1, ROWS, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, 0, FP, fr) == VS_ERR_ARG);
  CHECK(LAUNCH(&d, pcm, PITCH, (size_t)1 << 31, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(&d, pcm, (size_t)1 << 32, ROWS, (size_t)1 << 31, fs, len, gl, cy, CP, FP, fr) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, (size_t)1 << 31, FP, fr) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, (size_t)1 << 31, fr) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, 0, fr) == VS_ERR_ARG);
  o = d;
  o.span_q = 0;
  CHECK(LAUNCH(&o, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_RANGE);
  len[2] = NS + 1;
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_ARG);
  len[2] = -1;
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_ARG);
  len[2] = 3999;
  fs[4] = 0;
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, fr) == VS_ERR_RANGE);
  fs[4] = 22050;
  CHECK(launches == 0 && !staged);

  /* window_s == 0: one frame over each row, whatever its length */
  CHECK(LAUNCH(NULL, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, 1, fr) == VS_OK && launches == 1 && !staged);
  CHECK(seen.lpc.total_frames == ROWS && seen.lpc.n_lanes == ROWS && seen.lpc.pitch == PITCH && seen.lpc.frames_pitch == 1);
  CHECK(seen.lpc.pcm == pcm && seen.lpc.frames == fr && seen.lpc.formants == NULL && seen.lpc.coefs == cf && seen.counts == cnt);
  CHECK(seen.glottal == gl && seen.cycles == cy && seen.cycles_pitch == CP && seen.lpc.order == VS_ORDER);
  CHECK(seen.anchor == VS_CP_ANCHOR_CLOSE && seen.delay == 4 && seen.span_q == 77 && seen.min_equations == 0);
  for (int i = 0; i < ROWS; i++)
    CHECK(seen_rows[i].first == i && seen_rows[i].fs == fs[i] && seen_rows[i].L == len[i] && seen_rows[i].H == 0 &&
          seen_rows[i].s0 == 0 && seen_rows[i].n_frames == 1);
  CHECK(LAUNCH(&d, pcm, PITCH, ROWS, NS, fs, NULL, gl, cy, CP, FP, fr) == VS_OK && launches == 2);
  for (int i = 0; i < ROWS; i++) CHECK(seen_rows[i].L == NS && seen_rows[i].first == i);

  /* window_s > 0: the LPC analysis's rows; a row with more frames than frames_pitch is refused */
  o = d;
  o.window_s = 0.05;
  o.hop_s = 0.025;
  o.anchor = VS_CP_ANCHOR_GCI;
  o.delay = -9;
  o.min_equations = 50;
  CHECK(LAUNCH(&o, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, FP, fr) == VS_OK && launches == 3 && !staged);
  long total = 0;
  for (int i = 0; i < ROWS; i++) {
    CHECK(vs_cplpc_frames(&o, fs[i], len[i], &n) == VS_OK);
    CHECK(seen_rows[i].n_frames == n && seen_rows[i].first == total && seen_rows[i].s0 == 0);
    CHECK(seen_rows[i].L == (int32_t)floor(0.05 * fs[i] + 0.5) && seen_rows[i].H == (int32_t)floor(0.025 * fs[i] + 0.5));
    total += n;
  }
  CHECK(seen.lpc.total_frames == total && total == 9 + 0 + 18 + 0 + 3);
  CHECK(seen.anchor == VS_CP_ANCHOR_GCI && seen.delay == -9 && seen.min_equations == 50 && seen.lpc.pre == 0);
  CHECK(LAUNCH(&o, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, 17, fr) == VS_ERR_RANGE && launches == 3 && !staged);

  /* the host-buffer call: the same refusals, then the caller's arrays as the launch's */
  CHECK(vs_cplpc(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, 0, fr, NULL, cf, cnt) == VS_ERR_ARG);
  CHECK(vs_cplpc(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, 0, 1, fr, NULL, cf, cnt) == VS_ERR_ARG);
  CHECK(vs_cplpc(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, NULL, cy, CP, 1, fr, NULL, cf, cnt) == VS_ERR_ARG);
  CHECK(vs_cplpc(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, (size_t)1 << 31, fr, NULL, cf, cnt) == VS_ERR_UNSUPPORTED);
  o = d;
  o.delay = 40000;
  CHECK(vs_cplpc(ctx, &o, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, 1, fr, NULL, cf, cnt) == VS_ERR_RANGE && launches == 3);
  CHECK(vs_cplpc(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, gl, cy, CP, 1, fr, NULL, cf, NULL) == VS_OK && launches == 4);
  CHECK(seen.lpc.pcm == pcm && seen.glottal == gl && seen.cycles == cy && seen.lpc.frames == fr && seen.lpc.coefs == cf);
  CHECK(seen.lpc.formants == NULL && seen.counts == NULL && lpc_launches == 0 && !staged);

  /* the two plans of the one row upload at the smallest rows: lengths 0, 1 and n_samples, distinct rates */
  {
    int32_t fs3[3] = {8000, 16000, 22050}, len3[3] = {0, 1, NS};
    CHECK(LAUNCH(&d, pcm, PITCH, 3, NS, fs3, len3, gl, cy, CP, 1, fr) == VS_OK && launches == 5 && !staged);
    CHECK(seen_bytes == 3 * sizeof(VsLpcRow) && seen.lpc.total_frames == 3 && seen.lpc.n_lanes == 3);
    CHECK(seen.lpc.windows == NULL && seen.lpc.pre == 0);
    for (int i = 0; i < 3; i++) { /* first = i, fs, L = len, n_frames = 1, everything else 0: byte for byte */
      VsLpcRow want;
      memset(&want, 0, sizeof(want));
      want.first = i;
      want.fs = fs3[i];
      want.L = len3[i];
      want.n_frames = 1;
      CHECK(memcmp(&seen_rows[i], &want, sizeof(want)) == 0);
    }
    /* window_s > 0: the rows and one rectangular table per distinct L, ascending, as vs_lpc_launch stages them */
    o = d;
    o.window_s = 0.05;
    o.hop_s = 0.025;
    CHECK(LAUNCH(&o, pcm, PITCH, 3, NS, fs3, len3, gl, cy, CP, FP, fr) == VS_OK && launches == 6 && !staged);
    const int32_t L3[3] = {400, 800, 1103}; /* floor(0.05 fs + 0.5); the hop at 22050 Hz is 551 */
    CHECK(seen_bytes == 3 * sizeof(VsLpcRow) + (size_t)(L3[0] + L3[1] + L3[2]) * sizeof(int32_t));
    CHECK(seen.lpc.windows != NULL && seen.lpc.total_frames == 0 + 0 + 1 + (NS - 1103) / 551 && seen.lpc.pre == 0);
    for (int i = 0, woff = 0; i < 3; woff += L3[i], i++) {
      CHECK(seen_rows[i].L == L3[i] && seen_rows[i].woff == woff && seen_rows[i].fs == fs3[i] && seen_rows[i].s0 == 0);
      CHECK(seen_rows[i].n_frames == (i == 2 ? 1 + (NS - 1103) / 551 : 0) && seen_rows[i].first == 0);
      for (int k = 0; k < L3[i]; k++) CHECK(seen_win[woff + k] == 256);
    }
    /* row by row: a bad length answers before a bad rate behind it, and the other way round */
    int32_t fsb[3] = {8000, 16000, 0}, lenb[3] = {0, NS + 1, NS};
    CHECK(LAUNCH(&d, pcm, PITCH, 3, NS, fsb, lenb, gl, cy, CP, 1, fr) == VS_ERR_ARG);
    CHECK(LAUNCH(&o, pcm, PITCH, 3, NS, fsb, lenb, gl, cy, CP, FP, fr) == VS_ERR_ARG);
    fsb[0] = 0;
    CHECK(LAUNCH(&d, pcm, PITCH, 3, NS, fsb, lenb, gl, cy, CP, 1, fr) == VS_ERR_RANGE);
    CHECK(LAUNCH(&o, pcm, PITCH, 3, NS, fsb, lenb, gl, cy, CP, FP, fr) == VS_ERR_RANGE);
    lenb[0] = -1;
    CHECK(LAUNCH(&d, pcm, PITCH, 3, NS, fsb, lenb, gl, cy, CP, 1, fr) == VS_ERR_ARG && launches == 6 && !staged);
  }

  free(pcm);
  free(gl);
  free(cy);
  free(fr);
  free(cf);
  free(cnt);
  free(ctx);
  printf("ok\n");
  return 0;
}
