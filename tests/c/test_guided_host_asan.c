/*
 * test_guided_host_asan.c -- the device-free half of the guided marks (csrc/vs_guided_host.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer: the defaults, every refusal of the options, vs_guided_plan over the extreme rates and
 * lengths, and -- with stand-ins for the record upload, the block cache, the host-buffer call and the two launchers, which
 * only keep what they are handed -- the arguments vs_guided_launch and vs_guided refuse and the row records, scratch
 * layout and launch arguments they build.  Needs the HIP runtime's C header only.  Prints "ok".
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../voice_synth_amd/csrc/vs_internal.h"
#include "../../voice_synth_amd/csrc/vs_guided.h"
#include "../../voice_synth_amd/csrc/vs_pitch.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      exit(1);                                                     \
    }                                                              \
  } while (0)

/* ---- stand-ins ---- */
static void *staged;
static size_t staged_bytes;
static int blocks_out; /* blocks of the cache handed out and not yet retired */
static VsMgArgs seen;
static VsMgRow seen_rows[64];
static VsPtArgs seen_pt;
static int launches, pitch_launches;

int vs_rec_stage(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, void **host)
{
  CHECK(slot == &ctx->rec_guided || slot == &ctx->rec_pitch);
  free(staged);
  staged = malloc(bytes ? bytes : 1);
  staged_bytes = bytes;
  *host = staged;
  return VS_OK;
}
int vs_rec_upload(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, VsRecBlock *blk)
{
  CHECK(staged && bytes == staged_bytes);
  blk->dev = malloc(bytes ? bytes : 1); /* the device's copy */
  memcpy(blk->dev, staged, bytes);
  blk->cap = bytes;
  blocks_out++;
  return VS_OK;
}
hipError_t plan_block_get(vs_ctx *ctx, size_t bytes, void **ptr, size_t *cap)
{
  *ptr = malloc(bytes ? bytes : 1); /* exactly that size: a write past the stated layout is caught */
  *cap = bytes;
  blocks_out++;
  return *ptr ? hipSuccess : hipErrorOutOfMemory;
}
void plan_block_put(vs_ctx *ctx, void *ptr, size_t cap, VsRetire *retire)
{
  free(ptr);
  blocks_out--;
}
int vs_rec_retire(vs_ctx *ctx, VsRecBlock *blk, hipError_t launched)
{
  CHECK(blk->dev);
  free(blk->dev);
  blk->dev = NULL;
  blocks_out--;
  return launched == hipSuccess ? VS_OK : VS_ERR_HIP;
}
/* the records + scratch pair of csrc/vs_blocks.c, over the stand-ins above */
#include "rec_scratch_standin.h"
hipError_t vs_launch_guided(const VsMgArgs *a, hipStream_t s)
{
  seen = *a;
  CHECK(a->n_lanes <= 64);
  memcpy(seen_rows, a->rows, (size_t)a->n_lanes * sizeof(VsMgRow));
  /* the scratch as the kernels use it: the heads, lag and link of every row, to their last byte */
  memset(a->head, 0, (size_t)a->n_lanes * sizeof(VsMgHead));
  memset(a->lag, 0, (size_t)a->n_lanes * (size_t)a->frames_pitch * sizeof(int32_t));
  memset(a->link, 0, (size_t)a->n_lanes * (size_t)a->frames_pitch * sizeof(int32_t));
  launches++;
  return hipSuccess;
}
hipError_t vs_launch_pitch(const VsPtArgs *a, int lds_doubles, hipStream_t s)
{
  seen_pt = *a;
  pitch_launches++;
  return hipSuccess;
}
int vs_host_begin(vs_ctx *ctx, const void *in, size_t in_bytes, VsHostPart *parts, int n_parts)
{
  ctx->pool.d_in = (void *)in;
  for (int k = 0; k < n_parts; k++) parts[k].dev = parts[k].host && parts[k].bytes ? parts[k].host : NULL;
  return VS_OK;
}
int vs_host_end(vs_ctx *ctx, int launch_rc, const VsHostPart *parts, int n_parts) { return launch_rc; }

static int opts_rc(const vs_guided_opts *o) { return vs_guided_plan(o, 16000, 16000, NULL, NULL, NULL, NULL, NULL); }

int main(void)
{
  vs_guided_opts d, o;
  int32_t tmin = 0, tmax = 0, H = 0, n = 0, C = 0;
  CHECK(sizeof(vs_guided_opts) == 32 && sizeof(vs_guided_rec) == 16 && sizeof(vs_guided_seg) == 16);
  CHECK(sizeof(VsMgRow) == 32 && sizeof(VsMgHead) == 16);
  CHECK(vs_guided_defaults(NULL) == VS_ERR_ARG && vs_guided_defaults(&d) == VS_OK);
  CHECK(d.f0_min == 50.0f && d.f0_max == 500.0f && d.polarity == 1 && d.segments == VS_MG_ALL && d.edge_frames == 1);
  CHECK(d.min_frames == 3 && d.hop_s == 0.010);
  CHECK(vs_guided_plan(NULL, 16000, 16000, &tmin, &tmax, &H, &n, &C) == VS_OK);
  CHECK(tmin == 32 && tmax == 320 && H == 160 && n == 94 && C == 480);

  /* the options, each at its last good and its first bad value */
#define WITH(field, value) (o = d, o.field = (value), opts_rc(&o))
  CHECK(WITH(polarity, -1) == VS_OK && WITH(polarity, 0) == VS_ERR_ARG && WITH(polarity, 2) == VS_ERR_ARG);
  CHECK(WITH(segments, VS_MG_LONGEST) == VS_OK && WITH(segments, 2) == VS_ERR_ARG && WITH(segments, -1) == VS_ERR_ARG);
  CHECK(WITH(edge_frames, 0) == VS_OK && WITH(edge_frames, VS_MG_MAX_EDGE) == VS_OK);
  CHECK(WITH(edge_frames, -1) == VS_ERR_RANGE && WITH(edge_frames, VS_MG_MAX_EDGE + 1) == VS_ERR_RANGE);
  CHECK(WITH(min_frames, 1) == VS_OK && WITH(min_frames, 2147483647) == VS_OK && WITH(min_frames, 0) == VS_ERR_RANGE);
  CHECK(WITH(min_frames, -2147483647 - 1) == VS_ERR_RANGE);
  CHECK(WITH(f0_min, 0.0f) == VS_ERR_ARG && WITH(f0_max, NAN) == VS_ERR_ARG && WITH(f0_min, INFINITY) == VS_ERR_ARG);
  CHECK(WITH(hop_s, NAN) == VS_ERR_ARG && WITH(hop_s, INFINITY) == VS_ERR_ARG && WITH(hop_s, -0.01) == VS_ERR_ARG);
  CHECK(WITH(hop_s, 0.0) == VS_ERR_RANGE && WITH(hop_s, 0.00003) == VS_ERR_RANGE && WITH(hop_s, 0.000032) == VS_OK);
  CHECK(WITH(hop_s, 134217.0) == VS_OK && WITH(hop_s, 134218.0) == VS_ERR_RANGE && WITH(hop_s, 1e300) == VS_ERR_RANGE);
  CHECK(WITH(f0_min, 7.8f) == VS_ERR_RANGE && WITH(f0_max, 8001.0f) == VS_ERR_RANGE && WITH(f0_max, 50.0f) == VS_ERR_RANGE);
  o = d; /* an ARG fault is named before a RANGE fault */
  o.polarity = 3;
  o.edge_frames = 99;
  CHECK(opts_rc(&o) == VS_ERR_ARG);

  /* the row plan: the pitch track's frames at every length, the extreme rates */
  vs_pitch_opts pd;
  vs_pitch_defaults(&pd);
  const int32_t lens[] = {0, 961, 962, 1121, 1122, 16000, 2147483647};
  for (size_t k = 0; k < sizeof(lens) / sizeof(lens[0]); k++) {
    int32_t pn = -1;
    CHECK(vs_guided_plan(&d, 16000, lens[k], NULL, NULL, NULL, &n, NULL) == VS_OK);
    CHECK(vs_pitch_frames(&pd, 16000, lens[k], &pn) == VS_OK && pn == n);
  }
  CHECK(vs_guided_plan(&d, 0, 100, NULL, NULL, NULL, &n, NULL) == VS_ERR_RANGE);
  CHECK(vs_guided_plan(&d, 16000, -1, NULL, NULL, NULL, &n, NULL) == VS_ERR_RANGE);
  CHECK(vs_guided_plan(&d, 192000, 96000, NULL, NULL, NULL, &n, NULL) == VS_ERR_RANGE);
  CHECK(vs_guided_plan(&d, 999, 5000, NULL, NULL, NULL, &n, NULL) == VS_ERR_RANGE); /* tmin 1 */
  CHECK(vs_guided_plan(&d, 1000, 5000, &tmin, &tmax, &H, &n, &C) == VS_OK && tmin == 2 && tmax == 20 && H == 10 && C == 30);
  CHECK(vs_guided_plan(&d, 96000, 2147483647, &tmin, &tmax, &H, &n, &C) == VS_OK);
  CHECK(tmax == 1920 && H == 960 && C == 2880 && n == 1 + (2147483647 - 5762) / 960);
  o = d;
  o.f0_min = 47.0f;
  CHECK(vs_guided_plan(&o, 96000, 6200, &tmin, &tmax, &H, &n, &C) == VS_OK && tmax == 2043 && C == 3064 && n == 1);
  o = d;
  o.hop_s = 134217.0; /* the longest hop at the longest row: two frames */
  CHECK(vs_guided_plan(&o, 16000, 2147483647, NULL, NULL, &H, &n, NULL) == VS_OK && H == 2147472000 && n == 2);

  /* the launch: refusals before anything is staged, then the rows, the scratch and the arguments it builds */
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(struct vs_ctx));
  CHECK(ctx);
  enum { ROWS = 5, NS = 4000, PITCH = 4008, FP = 50, MP = 50, SP = 3 };
  int16_t *pcm = (int16_t *)calloc((size_t)ROWS * PITCH, sizeof(int16_t));
  vs_pitch_frame *fr = (vs_pitch_frame *)calloc((size_t)ROWS * FP, sizeof(vs_pitch_frame));
  vs_acoustic out[ROWS];
  vs_guided_rec rec[ROWS];
  vs_guided_seg segs[ROWS * SP];
  int32_t *marks = (int32_t *)calloc((size_t)ROWS * MP, sizeof(int32_t));
  CHECK(pcm && fr && marks);
  int32_t fs[ROWS] = {16000, 16000, 8000, 16000, 22050}, len[ROWS] = {4000, 0, 3999, 961, 2500};
#define LAUNCH(c, p, pi, nl, ns, f, l, frd, fp, od, md, mp, rd, sd, sp) \
  vs_guided_launch(c, &d, p, pi, nl, ns, f, l, frd, fp, od, md, mp, rd, sd, sp)
  CHECK(LAUNCH(NULL, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, NULL, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, NULL, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, NULL, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, 0, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, NULL, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, 0, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, NULL, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, 0) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, 0, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, 0, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, NS - 1, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, (vs_pitch_frame *)((char *)fr + 4), FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, (size_t)1 << 31, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(ctx, pcm, (size_t)1 << 32, ROWS, (size_t)1 << 31, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, (size_t)1 << 31, out, marks, MP, rec, segs, SP) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, (size_t)1 << 31, rec, segs, SP) == VS_ERR_UNSUPPORTED);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, (size_t)1 << 31) == VS_ERR_UNSUPPORTED);
  o = d;
  o.segments = 7;
  CHECK(vs_guided_launch(ctx, &o, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(launches == 0 && !staged && blocks_out == 0);
  len[2] = NS + 1;
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  len[2] = 3999;
  fs[4] = 0;
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_ERR_RANGE);
  fs[4] = 22050;
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, len, fr, 18, out, marks, MP, rec, segs, SP) == VS_ERR_RANGE); /* row 0 has 19 */
  CHECK(launches == 0 && blocks_out == 0);

  o = d;
  o.polarity = -1;
  o.segments = VS_MG_LONGEST;
  o.edge_frames = 2;
  o.min_frames = 5;
  CHECK(vs_guided_launch(ctx, &o, pcm, PITCH, ROWS, NS, fs, len, fr, FP, out, marks, MP, rec, segs, SP) == VS_OK);
  CHECK(launches == 1 && blocks_out == 0);
  CHECK(seen.pcm == pcm && seen.pitch == PITCH && seen.n_lanes == ROWS && seen.n_samples == NS && seen.frames == fr);
  CHECK(seen.frames_pitch == FP && seen.out == out && seen.marks == marks && seen.marks_pitch == MP && seen.rec == rec);
  CHECK(seen.segs == segs && seen.seg_pitch == SP && seen.polarity == -1 && seen.segments == VS_MG_LONGEST);
  CHECK(seen.edge_frames == 2 && seen.min_frames == 5);
  CHECK((char *)seen.lag == (char *)seen.head + ROWS * sizeof(VsMgHead) && seen.link == seen.lag + ROWS * FP);
  CHECK(vs_mg_scratch_bytes(ROWS, FP) == ROWS * 16 + 2 * ROWS * FP * 4);
  for (int i = 0; i < ROWS; i++) {
    const VsMgRow *r = &seen_rows[i];
    int32_t pn = -1;
    CHECK(vs_pitch_frames(&pd, fs[i], len[i], &pn) == VS_OK);
    CHECK(r->n_frames == pn && r->len == len[i] && r->fs == fs[i] && r->reserved_ == 0);
    CHECK(r->tmin == fs[i] / 500 && r->tmax == (fs[i] + 49) / 50 && r->H == (int32_t)floor(0.010 * fs[i] + 0.5));
    CHECK(r->C == r->tmax + r->tmax / 2);
  }
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, NS, fs, NULL, fr, FP, out, NULL, 0, rec, NULL, 0) == VS_OK && launches == 2);
  CHECK(seen.marks == NULL && seen.marks_pitch == 0 && seen.segs == NULL && seen.seg_pitch == 0 && blocks_out == 0);
  for (int i = 0; i < ROWS; i++) CHECK(seen_rows[i].len == NS);

  /* the host-buffer call: the same refusals, the track launched with the guided options' range and hop, the caller's
   * arrays as the launch's; without frames a block of the cache takes the records */
  CHECK(vs_guided(ctx, &d, NULL, pcm, PITCH, ROWS, NS, fs, len, 0, fr, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(vs_guided(ctx, &d, NULL, pcm, PITCH, ROWS, NS, fs, len, FP, fr, NULL, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(vs_guided(ctx, &d, NULL, pcm, PITCH, ROWS, NS, fs, len, FP, fr, out, marks, MP, rec, segs, 0) == VS_ERR_ARG);
  o = d;
  o.min_frames = 0;
  CHECK(vs_guided(ctx, &o, NULL, pcm, PITCH, ROWS, NS, fs, len, FP, fr, out, marks, MP, rec, segs, SP) == VS_ERR_RANGE);
  vs_pitch_opts po = pd;
  po.jump_q = -1;
  CHECK(vs_guided(ctx, &d, &po, pcm, PITCH, ROWS, NS, fs, len, FP, fr, out, marks, MP, rec, segs, SP) == VS_ERR_ARG);
  CHECK(launches == 2 && pitch_launches == 0 && blocks_out == 0);
  po = pd;
  po.octave_q = 3277;
  po.f0_min = 99.0f; /* replaced by the guided options' */
  o = d;
  o.f0_min = 70.0f;
  o.hop_s = 0.005;
  CHECK(vs_guided(ctx, &o, &po, pcm, PITCH, ROWS, NS, fs, len, 64, fr, out, marks, MP, rec, segs, SP) == VS_ERR_RANGE); /* row 2 has 92 */
  free(fr);
  fr = (vs_pitch_frame *)calloc((size_t)ROWS * 128, sizeof(vs_pitch_frame));
  CHECK(fr);
  pitch_launches = 0;
  CHECK(vs_guided(ctx, &o, &po, pcm, PITCH, ROWS, NS, fs, len, 128, fr, out, marks, MP, rec, segs, SP) == VS_OK);
  CHECK(launches == 3 && pitch_launches == 1 && blocks_out == 0);
  CHECK(seen_pt.octave_q == 3277 && seen_pt.frames == fr && seen.frames == fr && seen.pcm == pcm && seen.out == out);
  CHECK(seen_rows[0].tmax == 229 && seen_rows[0].H == 80 && seen_rows[0].n_frames == 1 + (4000 - 689) / 80);
  CHECK(vs_guided(ctx, NULL, NULL, pcm, PITCH, ROWS, NS, fs, len, FP, NULL, out, NULL, 0, rec, NULL, 0) == VS_OK);
  CHECK(launches == 4 && pitch_launches == 2 && blocks_out == 0 && seen.frames == seen_pt.frames && seen.frames != fr);

  free(staged);
  free(pcm);
  free(fr);
  free(marks);
  free(ctx);
  printf("ok\n");
  return 0;
}
