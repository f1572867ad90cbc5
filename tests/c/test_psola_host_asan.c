/*
 * test_psola_host_asan.c -- the device-free half of PSOLA (csrc/vs_psola_host.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer: the defaults, every refusal of the sizes, strides and options in their order, the tiles and
 * the scratch of the extreme sizes, and -- with stand-ins for the record upload, the block cache, the host-buffer call and
 * the launcher, which only keep what they are handed -- the arguments vs_psola_launch and vs_psola refuse and the row
 * records, the scratch and the launch arguments they build.  Needs the HIP runtime's C header only.  Prints "ok".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../voice_synth_amd/csrc/vs_internal.h"
#include "../../voice_synth_amd/csrc/vs_psola.h"

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
static VsPsArgs seen;
static VsPsRow seen_rows[64];
static int launches;
static hipError_t launch_answer = hipSuccess;

int vs_rec_stage(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, void **host)
{
  CHECK(slot == &ctx->rec_psola);
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
hipError_t vs_launch_psola(const VsPsArgs *a, hipStream_t s)
{
  seen = *a;
  CHECK(a->c.n_lanes <= 64);
  memcpy(seen_rows, a->rows, (size_t)a->c.n_lanes * sizeof(VsPsRow));
  /* the scratch as the kernels use it: a VsPsAux next to every synthesis mark, to the last byte */
  memset(a->aux, 0, (size_t)a->c.n_lanes * (size_t)a->c.synth_pitch * sizeof(VsPsAux));
  launches++;
  return launch_answer;
}
int vs_host_begin(vs_ctx *ctx, const void *in, size_t in_bytes, VsHostPart *parts, int n_parts)
{
  ctx->pool.d_in = (void *)in;
  for (int k = 0; k < n_parts; k++) parts[k].dev = parts[k].host && parts[k].bytes ? parts[k].host : NULL;
  return VS_OK;
}
int vs_host_end(vs_ctx *ctx, int launch_rc, const VsHostPart *parts, int n_parts) { return launch_rc; }

int main(void)
{
  vs_psola_opts d, o, r;
  CHECK(sizeof(vs_psola_opts) == 16 && sizeof(vs_psola_mark) == 16 && sizeof(vs_psola_stat) == 24);
  CHECK(sizeof(VsPsRow) == 4 && sizeof(VsPsAux) == 8 && VS_PS_TILE == 2048 && VS_PS_LDS == 4112);
  CHECK(vs_psola_defaults(NULL) == VS_ERR_ARG && vs_psola_defaults(&d) == VS_OK);
  CHECK(d.pmin == 32 && d.pmax == 320 && d.reserved_[0] == 0 && d.reserved_[1] == 0);

  /* the check, every argument at its last good and its first bad value: ARG, then UNSUPPORTED, then RANGE */
#define CK(op, pi, nl, ns, mp, hs, sgp, ss, ps, hg, gs, cs, tp, opi, sp) \
  vs_psola_check(op, pi, nl, ns, mp, hs, sgp, ss, ps, hg, gs, cs, tp, opi, sp, &r)
  const size_t BIG = (size_t)1 << 31;
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_OK && r.pmin == 32 && r.pmax == 320);
  CHECK(CK(NULL, 100, 0, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 0, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 0, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 0, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 99, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 99, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 1) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 1, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 1, 1, 4, 4, 0, 0, 4, 1, 100, 2) == VS_OK);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 0, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 2, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 6, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 3, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 1, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 7, 4, 1, 100, 2) == VS_OK); /* no gains: their stride is not read */
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 32, 32, 1, 96, 24, 1, 100, 2) == VS_OK);
  o = d;
  o.reserved_[1] = 1;
  CHECK(CK(&o, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_ARG);
  CHECK(CK(NULL, BIG, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, 100, BIG, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, BIG, 1, BIG, 1, 0, 0, 4, 4, 0, 0, 4, 1, BIG, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, 100, 1, 100, BIG, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, 100, 1, 100, 1, 1, BIG, 4, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, BIG, 4, 0, 0, 4, 1, 100, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, BIG, 100, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, BIG) == VS_ERR_UNSUPPORTED);
  /* one workgroup per (row, tile): 2^20 rows of 2^22 samples are 2^31 + 2^20 of them */
  CHECK(CK(NULL, (size_t)1 << 22, (size_t)1 << 20, (size_t)1 << 22, 1, 0, 0, 4, 4, 0, 0, 4, 1, (size_t)1 << 22, 2) == VS_ERR_UNSUPPORTED);
  CHECK(CK(NULL, (size_t)1 << 21, (size_t)1 << 20, (size_t)1 << 21, 1, 0, 0, 4, 4, 0, 0, 4, 1, (size_t)1 << 21, 2) == VS_OK);
#define WITH(field, value) (o = d, o.field = (value), CK(&o, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 2))
  CHECK(WITH(pmin, 2) == VS_OK && WITH(pmin, 1) == VS_ERR_RANGE && WITH(pmin, 320) == VS_OK && WITH(pmin, 321) == VS_ERR_RANGE);
  CHECK(WITH(pmax, VS_AC_MAX_LAG) == VS_OK && WITH(pmax, VS_AC_MAX_LAG + 1) == VS_ERR_RANGE && WITH(pmax, 31) == VS_ERR_RANGE);
  CHECK(WITH(pmin, -2147483647 - 1) == VS_ERR_RANGE && WITH(pmax, 2147483647) == VS_ERR_RANGE);
  o = d; /* an ARG fault is named before a RANGE fault */
  o.pmin = 0;
  CHECK(CK(&o, 100, 1, 100, 1, 0, 0, 4, 4, 0, 0, 4, 1, 100, 1) == VS_ERR_ARG);

  /* the tiles: a row may begin up to 7 samples behind a 16-byte address; the scratch */
  CHECK(vs_psola_tiles(1) == 1 && vs_psola_tiles(2041) == 1 && vs_psola_tiles(2042) == 2 && vs_psola_tiles(16000) == 8);
  CHECK(vs_psola_tiles(2147483647) == 1048577);
  CHECK(vs_psola_scratch_bytes(3, 7) == 3 * 7 * 8 && vs_psola_scratch_bytes(65536, 512) == (size_t)65536 * 512 * 8);

  /* the rows */
  VsPsRow rows[4];
  const int32_t good[4] = {0, 1, 99, 100}, over[4] = {0, 1, 101, 100}, under[4] = {0, -1, 99, 100};
  CHECK(vs_psola_fill(good, 4, 100, rows) == VS_OK && rows[0].length == 0 && rows[2].length == 99 && rows[3].length == 100);
  CHECK(vs_psola_fill(over, 4, 100, rows) == VS_ERR_RANGE && vs_psola_fill(under, 4, 100, rows) == VS_ERR_RANGE);
  CHECK(vs_psola_fill(NULL, 4, 100, rows) == VS_OK && rows[0].length == 100 && rows[3].length == 100);

  /* the launch: refusals before anything is staged, then the rows, the scratch and the arguments it builds */
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(struct vs_ctx));
  CHECK(ctx);
  enum { ROWS = 5, NS = 4000, PITCH = 4008, OP = 4003, MP = 50, SGP = 3, TP = 40, SP = 60 };
  int16_t *pcm = (int16_t *)calloc((size_t)ROWS * PITCH, sizeof(int16_t));
  int16_t *out = (int16_t *)calloc((size_t)ROWS * OP, sizeof(int16_t));
  int32_t *marks = (int32_t *)calloc((size_t)ROWS * MP, sizeof(int32_t));
  vs_strack_cycle *cyc = (vs_strack_cycle *)calloc((size_t)ROWS * TP, sizeof(vs_strack_cycle));
  int32_t *gain = (int32_t *)calloc((size_t)ROWS * TP, sizeof(int32_t));
  vs_psola_mark *synth = (vs_psola_mark *)calloc((size_t)ROWS * SP, sizeof(vs_psola_mark));
  vs_strack_stat sst[ROWS];
  vs_guided_rec rec[ROWS];
  vs_guided_seg segs[ROWS * SGP];
  vs_psola_stat stat[ROWS];
  CHECK(pcm && out && marks && cyc && gain && synth);
  memset(sst, 0, sizeof(sst));
  memset(rec, 0, sizeof(rec));
  memset(segs, 0, sizeof(segs));
  int32_t len[ROWS] = {4000, 0, 3999, 1, 2500};
  const int32_t *st_ = &cyc->start, *pe_ = &cyc->T, *cn_ = &sst->n_cycles;
#define LAUNCH(c, p, pi, nl, l, md, rd, sd, sgp, s0, ss, p0, ps, g0, gs, c0, cs, od, opi, std, syd, sp) \
  vs_psola_launch(c, &d, p, pi, nl, NS, l, md, MP, rd, sd, sgp, s0, ss, p0, ps, g0, gs, c0, cs, TP, od, opi, std, syd, sp)
  CHECK(LAUNCH(NULL, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, NULL, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, NULL, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, NULL, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, NULL, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, NULL, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, NULL, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, NULL, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, NULL, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, NULL, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, 0, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 30, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 2, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, NS - 1, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, 1) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, (int16_t *)((char *)pcm + 1), PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, (const int32_t *)((const char *)st_ + 2), 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, pcm, PITCH, BIG, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_UNSUPPORTED);
  CHECK(launches == 0 && !staged && blocks_out == 0);
  len[2] = NS + 1;
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_RANGE);
  len[2] = -1;
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_RANGE);
  len[2] = 3999;
  CHECK(launches == 0 && blocks_out == 0);

  o = d;
  o.pmin = 20;
  o.pmax = 400;
  CHECK(vs_psola_launch(ctx, &o, pcm, PITCH, ROWS, NS, len, marks, MP, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, TP,
                        out + 1, OP, stat, synth, SP) == VS_OK);
  CHECK(launches == 1 && blocks_out == 0);
  CHECK(seen.c.pcm == pcm && seen.c.pitch == PITCH && seen.c.n_lanes == ROWS && seen.n_samples == NS && seen.c.marks == marks);
  CHECK(seen.c.marks_pitch == MP && seen.c.rec == rec && seen.c.segs == segs && seen.c.seg_pitch == SGP);
  CHECK(seen.c.start == (const char *)cyc && seen.c.period == (const char *)cyc + 4 && seen.c.gain == (const char *)gain);
  CHECK(seen.c.count == (const char *)sst + 4 && seen.c.start_stride == 32 && seen.c.period_stride == 32 && seen.c.gain_stride == 4);
  CHECK(seen.c.count_stride == 24 && seen.c.target_pitch == TP && seen.c.out == out + 1 && seen.c.out_pitch == OP);
  CHECK(seen.c.stat == stat && seen.c.synth == synth && seen.c.synth_pitch == SP && seen.c.pmin == 20 && seen.c.pmax == 400);
  for (int i = 0; i < ROWS; i++) CHECK(seen_rows[i].length == len[i]);
  /* no lengths, no segment records, no gains */
  CHECK(vs_psola_launch(ctx, NULL, pcm, PITCH, ROWS, NS, NULL, marks, MP, rec, NULL, 9, st_, 32, pe_, 32, NULL, 9, cn_, 24, TP, out,
                        OP, stat, synth, SP) == VS_OK);
  CHECK(launches == 2 && blocks_out == 0 && seen.c.segs == NULL && seen.c.seg_pitch == 0 && seen.c.gain == NULL);
  CHECK(seen.c.gain_stride == 0 && seen.c.pmin == 32 && seen.c.pmax == 320);
  for (int i = 0; i < ROWS; i++) CHECK(seen_rows[i].length == NS);
  /* a launch that fails: both blocks are given back */
  launch_answer = hipErrorInvalidValue;
  CHECK(LAUNCH(ctx, pcm, PITCH, ROWS, len, marks, rec, segs, SGP, st_, 32, pe_, 32, gain, 4, cn_, 24, out, OP, stat, synth, SP) == VS_ERR_HIP);
  CHECK(launches == 3 && blocks_out == 0);
  launch_answer = hipSuccess;

  /* the host-buffer call: the same refusals, dense arrays at stride 4, the caller's arrays as the launch's */
  int32_t *start = (int32_t *)calloc((size_t)ROWS * TP, sizeof(int32_t)), *period = (int32_t *)calloc((size_t)ROWS * TP, sizeof(int32_t));
  int32_t count[ROWS] = {0, 1, TP, TP + 1, -1};
  int16_t *y = (int16_t *)calloc((size_t)ROWS * NS, sizeof(int16_t));
  CHECK(start && period && y);
#define HOST(p, l, sd, sgp, g0, yd, sp) \
  vs_psola(ctx, NULL, p, PITCH, ROWS, NS, l, marks, MP, rec, sd, sgp, start, period, g0, count, TP, yd, stat, synth, sp)
  CHECK(HOST(NULL, len, segs, SGP, gain, y, SP) == VS_ERR_ARG && HOST(pcm, len, segs, SGP, gain, NULL, SP) == VS_ERR_ARG);
  CHECK(HOST(pcm, len, segs, 0, gain, y, SP) == VS_ERR_ARG && HOST(pcm, len, segs, SGP, gain, y, 1) == VS_ERR_ARG);
  len[4] = NS + 1;
  CHECK(HOST(pcm, len, segs, SGP, gain, y, SP) == VS_ERR_RANGE && launches == 3 && blocks_out == 0);
  len[4] = 2500;
  CHECK(HOST(pcm, len, segs, SGP, gain, y, SP) == VS_OK && launches == 4 && blocks_out == 0);
  CHECK(seen.c.pcm == pcm && seen.c.out == y && seen.c.out_pitch == NS && seen.c.start == (const char *)start);
  CHECK(seen.c.period == (const char *)period && seen.c.gain == (const char *)gain && seen.c.count == (const char *)count);
  CHECK(seen.c.start_stride == 4 && seen.c.period_stride == 4 && seen.c.gain_stride == 4 && seen.c.count_stride == 4);
  CHECK(seen.c.segs == segs && seen.c.seg_pitch == SGP && seen.c.synth == synth && seen.c.stat == stat);
  CHECK(HOST(pcm, NULL, NULL, 0, NULL, y, SP) == VS_OK && launches == 5 && seen.c.segs == NULL && seen.c.gain == NULL);

  free(staged);
  free(pcm);
  free(out);
  free(marks);
  free(cyc);
  free(gain);
  free(synth);
  free(start);
  free(period);
  free(y);
  free(ctx);
  printf("ok\n");
  return 0;
}
