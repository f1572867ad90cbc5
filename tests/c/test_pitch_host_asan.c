/*
 * test_pitch_host_asan.c -- the device-free half of the pitch track (csrc/vs_pitch_host.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer: the defaults, every refusal of the options, vs_pitch_frames, the Lg table, and -- with
 * stand-ins for the record upload, the host-buffer call and the launcher, which only keep what they are handed -- the
 * arguments vs_pitch_launch and vs_pitch refuse and the row records, table and launch arguments they build.  Needs the
 * HIP runtime's C header only.  Prints "ok".
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../voice_synth_amd/csrc/vs_internal.h"
#include "../../voice_synth_amd/csrc/vs_pitch.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      exit(1);                                                     \
    }                                                              \
  } while (0)

/* ---- stand-ins: the record upload keeps the staged bytes in a block of exactly that size, the launcher copies the
 * arguments, the rows and the table it was given, the host-buffer call hands the caller's arrays through ---- */
static void *staged;
static size_t staged_bytes;
static VsPtArgs seen;
static VsPtRow seen_rows[64];
static int32_t seen_lg[VS_AC_MAX_LAG + 1];
static int seen_lds, launches;

int vs_rec_stage(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, void **host)
{
  CHECK(slot == &ctx->rec_pitch);
  free(staged); /* (a launch that is refused row by row leaves its staged block to the slot) */
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
hipError_t vs_launch_pitch(const VsPtArgs *a, int lds_doubles, hipStream_t s)
{
  seen = *a;
  seen_lds = lds_doubles;
  CHECK(a->n_lanes <= 64 && (size_t)a->n_lanes * sizeof(VsPtRow) + sizeof(seen_lg) == staged_bytes);
  CHECK((const void *)a->rows == staged && (const char *)a->lg == (const char *)staged + a->n_lanes * sizeof(VsPtRow));
  memcpy(seen_rows, a->rows, (size_t)a->n_lanes * sizeof(VsPtRow));
  memcpy(seen_lg, a->lg, sizeof(seen_lg));
  launches++;
  return hipSuccess;
}
int vs_host_begin(vs_ctx *ctx, const void *in, size_t in_bytes, VsHostPart *parts, int n_parts)
{
  ctx->pool.d_in = (void *)in;
  for (int k = 0; k < n_parts; k++) parts[k].dev = parts[k].host && parts[k].bytes ? parts[k].host : NULL;
  return VS_OK;
}
int vs_host_end(vs_ctx *ctx, int launch_rc, const VsHostPart *parts, int n_parts) { return launch_rc; }

static int opts_rc(const vs_pitch_opts *o)
{
  int32_t n = -7;
  return vs_pitch_frames(o, 16000, 16000, &n);
}

int main(void)
{
  vs_pitch_opts d, o;
  int32_t n = 0;
  CHECK(sizeof(vs_pitch_opts) == 40 && sizeof(vs_pitch_frame) == 96 && sizeof(VsPtRow) == 32);
  CHECK(vs_pitch_defaults(NULL) == VS_ERR_ARG && vs_pitch_defaults(&d) == VS_OK);
  CHECK(d.f0_min == 50.0f && d.f0_max == 500.0f && d.voicing_q == 14746 && d.octave_q == 328 && d.jump_q == 11469);
  CHECK(d.vuv_q == 4588 && d.silence_rms == 16 && d.hop_s == 0.010 && d.reserved_ == 0);
  CHECK(vs_pitch_frames(&d, 16000, 16000, NULL) == VS_ERR_ARG);
  CHECK(vs_pitch_frames(NULL, 16000, 16000, &n) == VS_OK && n == 94);

  /* the ranges, each at its last good and its first bad value */
#define WITH(field, value) (o = d, o.field = (value), opts_rc(&o))
  CHECK(WITH(voicing_q, 0) == VS_OK && WITH(voicing_q, VS_PT_MAX_COST) == VS_OK);
  CHECK(WITH(voicing_q, -1) == VS_ERR_ARG && WITH(voicing_q, VS_PT_MAX_COST + 1) == VS_ERR_ARG);
  CHECK(WITH(octave_q, VS_PT_MAX_COST) == VS_OK && WITH(octave_q, -2147483647 - 1) == VS_ERR_ARG);
  CHECK(WITH(jump_q, 0) == VS_OK && WITH(jump_q, 2147483647) == VS_ERR_ARG);
  CHECK(WITH(vuv_q, VS_PT_MAX_COST) == VS_OK && WITH(vuv_q, -1) == VS_ERR_ARG);
  CHECK(WITH(silence_rms, 0) == VS_OK && WITH(silence_rms, 32767) == VS_OK);
  CHECK(WITH(silence_rms, -1) == VS_ERR_ARG && WITH(silence_rms, 32768) == VS_ERR_ARG && WITH(reserved_, 1) == VS_ERR_ARG);
  CHECK(WITH(f0_min, 0.0f) == VS_ERR_ARG && WITH(f0_max, NAN) == VS_ERR_ARG && WITH(f0_min, INFINITY) == VS_ERR_ARG);
  CHECK(WITH(hop_s, NAN) == VS_ERR_ARG && WITH(hop_s, INFINITY) == VS_ERR_ARG && WITH(hop_s, -0.01) == VS_ERR_ARG);
  CHECK(WITH(hop_s, 0.0) == VS_ERR_RANGE && WITH(hop_s, 0.00003) == VS_ERR_RANGE && WITH(hop_s, 0.000032) == VS_OK);
  CHECK(WITH(hop_s, 134217.0) == VS_OK && WITH(hop_s, 134218.0) == VS_ERR_RANGE && WITH(hop_s, 1e300) == VS_ERR_RANGE);
  CHECK(WITH(f0_min, 7.8f) == VS_ERR_RANGE && WITH(f0_max, 8001.0f) == VS_ERR_RANGE && WITH(f0_max, 50.0f) == VS_ERR_RANGE);

  /* frames: none below 3*tmax + 2 samples, one more every H */
  const int32_t lens[] = {0, 961, 962, 1121, 1122, 16000, 2147483647};
  for (size_t k = 0; k < sizeof(lens) / sizeof(lens[0]); k++) {
    CHECK(vs_pitch_frames(&d, 16000, lens[k], &n) == VS_OK);
    CHECK(n == (lens[k] >= 962 ? 1 + (lens[k] - 962) / 160 : 0));
  }
  CHECK(vs_pitch_frames(&d, 0, 100, &n) == VS_ERR_RANGE && vs_pitch_frames(&d, 16000, -1, &n) == VS_ERR_RANGE);
  CHECK(vs_pitch_frames(&d, 96000, 96000, &n) == VS_OK && n == 1 + (96000 - 5762) / 960);
  CHECK(vs_pitch_frames(&d, 192000, 96000, &n) == VS_ERR_RANGE);

  /* the table */
  int32_t lg[VS_AC_MAX_LAG + 1];
  CHECK(vs_pitch_log2_table(0, lg) == VS_ERR_ARG && vs_pitch_log2_table(VS_AC_MAX_LAG + 2, lg) == VS_ERR_ARG);
  CHECK(vs_pitch_log2_table(5, NULL) == VS_ERR_ARG && vs_pitch_log2_table(1, lg) == VS_OK && lg[0] == 0);
  CHECK(vs_pitch_log2_table(VS_AC_MAX_LAG + 1, lg) == VS_OK && lg[1] == 0 && lg[2] == 256 && lg[3] == 406 && lg[2048] == 2816);

  /* the launch: refusals before anything is staged, then the rows and arguments it builds */
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(struct vs_ctx));
  CHECK(ctx);
  enum { ROWS = 5, NS = 4000, PITCH = 4008, FP = 50 };
  int16_t *pcm = (int16_t *)calloc((size_t)ROWS * PITCH, sizeof(int16_t));
  vs_pitch_frame *fr = (vs_pitch_frame *)calloc((size_t)ROWS * FP, sizeof(vs_pitch_frame));
  CHECK(pcm && fr);
  int32_t fs[ROWS] = {16000, 16000, 8000, 16000, 22050}, len[ROWS] = {4000, 0, 3999, 961, 2500};
  CHECK(vs_pitch_launch(NULL, &d, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, NULL, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, NULL, len, FP, fr) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, FP, NULL) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, 0, fr) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, 0, NS, fs, len, FP, fr) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, 0, fs, len, FP, fr) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, NS - 1, ROWS, NS, fs, len, FP, fr) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, FP, (vs_pitch_frame *)((char *)fr + 4)) == VS_ERR_ARG);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, (size_t)1 << 31, NS, fs, len, FP, fr) == VS_ERR_UNSUPPORTED);
  CHECK(vs_pitch_launch(ctx, &d, pcm, (size_t)1 << 32, ROWS, (size_t)1 << 31, fs, len, FP, fr) == VS_ERR_UNSUPPORTED);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, (size_t)1 << 31, fr) == VS_ERR_UNSUPPORTED);
  o = d;
  o.vuv_q = -1;
  CHECK(vs_pitch_launch(ctx, &o, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_ARG);
  CHECK(launches == 0 && !staged);
  len[2] = NS + 1;
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_ARG);
  len[2] = -1;
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_ARG);
  len[2] = 3999;
  fs[4] = 0;
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_RANGE);
  fs[4] = 22050;
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, 18, fr) == VS_ERR_RANGE && launches == 0); /* row 0 has 19 */

  CHECK(vs_pitch_launch(ctx, NULL, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_OK && launches == 1 && !staged);
  CHECK(seen.pcm == pcm && seen.pitch == PITCH && seen.n_lanes == ROWS && seen.frames == fr && seen.frames_pitch == FP);
  CHECK(seen.voicing_q == 14746 && seen.octave_q == 328 && seen.jump_q == 11469 && seen.vuv_q == 4588 && seen.silence_rms == 16);
  CHECK(memcmp(seen_lg, lg, sizeof(lg)) == 0);
  int64_t total = 0;
  int lds = 0;
  for (int i = 0; i < ROWS; i++) {
    const VsPtRow *r = &seen_rows[i];
    CHECK(vs_pitch_frames(&d, fs[i], len[i], &n) == VS_OK);
    CHECK(r->first == total && r->n_frames == n && r->len == len[i] && r->fs == fs[i]);
    CHECK(r->tmin == fs[i] / 500 && r->tmax == (fs[i] + 49) / 50 && r->H == (int32_t)floor(0.010 * fs[i] + 0.5));
    total += n;
    if (vs_pt_lds_doubles(r->tmin, r->tmax) > lds) lds = vs_pt_lds_doubles(r->tmin, r->tmax);
  }
  CHECK(seen.total_frames == total && total == 19 + 0 + 44 + 0 + 6 && seen_lds == lds);
  CHECK(vs_pt_lds_doubles(32, 320) * 8 == 18384 && vs_pt_lds_doubles(2, 2048) * 8 == 90384);
  CHECK(vs_pitch_launch(ctx, &d, pcm, PITCH, ROWS, NS, fs, NULL, FP, fr) == VS_OK && launches == 2);
  for (int i = 0; i < ROWS; i++) CHECK(seen_rows[i].len == NS);

  /* the host-buffer call: the same refusals, then the caller's arrays as the launch's */
  CHECK(vs_pitch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, 0, fr) == VS_ERR_ARG);
  CHECK(vs_pitch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, FP, NULL) == VS_ERR_ARG);
  CHECK(vs_pitch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, (size_t)1 << 31, fr) == VS_ERR_UNSUPPORTED);
  o = d;
  o.silence_rms = 40000;
  CHECK(vs_pitch(ctx, &o, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_ARG && launches == 2);
  o = d;
  o.hop_s = 0.001;
  CHECK(vs_pitch(ctx, &o, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_ERR_RANGE && launches == 2);
  CHECK(vs_pitch(ctx, &d, pcm, PITCH, ROWS, NS, fs, len, FP, fr) == VS_OK && launches == 3 && !staged);
  CHECK(seen.pcm == pcm && seen.frames == fr);

  free(staged);
  free(pcm);
  free(fr);
  free(ctx);
  printf("ok\n");
  return 0;
}
