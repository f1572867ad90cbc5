/*
 * test_strack_host_asan.c -- the device-free half of the source track (csrc/vs_strack_host.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer: the defaults, every refusal of the options, the sizes and the rows, the row that plays the
 * pitch track's frames, which cos rows a call needs and the size and layout of the uploaded block, and -- with stand-ins
 * for the record upload, the host-buffer call and the launcher, which only keep what they are handed -- the block and the
 * launch arguments vs_strack_launch and vs_strack build.  The block is allocated at exactly its stated size, so a write
 * past the layout is caught.  Needs the HIP runtime's C header only.  Prints "ok".
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../voice_synth_amd/csrc/vs_internal.h"
#include "../../voice_synth_amd/csrc/vs_pitch.h"
#include "../../voice_synth_amd/csrc/vs_strack.h"

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
static int blocks_out, launches;
static VsStArgs seen;
static void *seen_block; /* a copy of the block the launch saw */
static size_t seen_bytes;

int vs_rec_stage(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, void **host)
{
  CHECK(slot == &ctx->rec_strack);
  free(staged);
  staged = malloc(bytes ? bytes : 1);
  staged_bytes = bytes;
  *host = staged;
  return VS_OK;
}
int vs_rec_upload(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, VsRecBlock *blk)
{
  CHECK(slot == &ctx->rec_strack && staged && bytes == staged_bytes);
  blk->dev = malloc(bytes ? bytes : 1);
  memcpy(blk->dev, staged, bytes);
  blk->cap = bytes;
  blocks_out++;
  return VS_OK;
}
int vs_rec_retire(vs_ctx *ctx, VsRecBlock *blk, hipError_t launched)
{
  CHECK(blk->dev);
  free(blk->dev);
  blk->dev = NULL;
  blocks_out--;
  return launched == hipSuccess ? VS_OK : VS_ERR_HIP;
}
hipError_t vs_launch_strack(const VsStArgs *a, hipStream_t s)
{
  seen = *a;
  free(seen_block);
  seen_bytes = staged_bytes;
  seen_block = malloc(seen_bytes);
  memcpy(seen_block, a->rows, seen_bytes); /* the block begins with the rows */
  launches++;
  return hipSuccess;
}
hipError_t vs_launch_pitch(const VsPtArgs *a, int lds_doubles, hipStream_t s) { return hipSuccess; }
int vs_host_begin(vs_ctx *ctx, const void *in, size_t in_bytes, VsHostPart *parts, int n_parts)
{
  ctx->pool.d_in = (void *)in;
  for (int k = 0; k < n_parts; k++) parts[k].dev = parts[k].host && parts[k].bytes ? parts[k].host : NULL;
  return VS_OK;
}
int vs_host_end(vs_ctx *ctx, int launch_rc, const VsHostPart *parts, int n_parts) { return launch_rc; }
/* cos(PI*k/T2) as csrc/vs_planhost.c has it */
void vs_cos_row(int T2, double *row)
{
  for (int k = 0; k < T2; k++) row[k] = cos(4.0 * atan(1.0) * k / T2);
}

static int t2(float cq, int P) { return (int)ceil(0.5 * cq * P); }

int main(void)
{
  vs_strack_opts d, o;
  CHECK(sizeof(vs_strack_opts) == 8 && sizeof(vs_strack_row) == 24 && sizeof(vs_strack_cycle) == 32);
  CHECK(sizeof(vs_strack_stat) == 24 && sizeof(VsStRow) == 80 && VS_ST_LDS == 10240 && VS_ST_T2_MAX == 1025);
  CHECK(vs_strack_defaults(NULL) == VS_ERR_ARG && vs_strack_defaults(&d) == VS_OK && d.max_reject == 256 && d.reserved_ == 0);

  /* the sizes, the strides and the options: ARG before UNSUPPORTED before RANGE */
#define CHK(opts, nl, ns, ps, fp, ha, as, op, hc, cp) vs_strack_check(opts, nl, ns, ps, fp, ha, as, op, hc, cp, &o)
  CHECK(CHK(NULL, 4, 100, 4, 8, 0, 0, 100, 0, 0) == VS_OK && o.max_reject == 256);
  CHECK(CHK(&d, 0, 100, 4, 8, 0, 0, 100, 0, 0) == VS_ERR_ARG && CHK(&d, 4, 0, 4, 8, 0, 0, 100, 0, 0) == VS_ERR_ARG);
  CHECK(CHK(&d, 4, 100, 4, 0, 0, 0, 100, 0, 0) == VS_ERR_ARG && CHK(&d, 4, 100, 4, 8, 0, 0, 99, 0, 0) == VS_ERR_ARG);
  CHECK(CHK(&d, 4, 100, 0, 8, 0, 0, 100, 0, 0) == VS_ERR_ARG && CHK(&d, 4, 100, 6, 8, 0, 0, 100, 0, 0) == VS_ERR_ARG);
  CHECK(CHK(&d, 4, 100, 96, 8, 1, 2, 100, 0, 0) == VS_ERR_ARG && CHK(&d, 4, 100, 96, 8, 1, 8, 100, 0, 0) == VS_OK);
  CHECK(CHK(&d, 4, 100, 96, 8, 0, 3, 100, 0, 0) == VS_OK); /* without an amplitude track its stride is not looked at */
  CHECK(CHK(&d, 4, 100, 4, 8, 0, 0, 100, 1, 0) == VS_ERR_ARG && CHK(&d, 4, 100, 4, 8, 0, 0, 100, 1, 1) == VS_OK);
  CHECK(CHK(&d, (size_t)1 << 31, 100, 4, 8, 0, 0, 100, 0, 0) == VS_ERR_UNSUPPORTED);
  CHECK(CHK(&d, 4, (size_t)1 << 31, 4, 8, 0, 0, (size_t)1 << 31, 0, 0) == VS_ERR_UNSUPPORTED);
  CHECK(CHK(&d, 4, 100, 4, (size_t)1 << 31, 0, 0, 100, 0, 0) == VS_ERR_UNSUPPORTED);
  CHECK(CHK(&d, 4, 100, (size_t)1 << 31, 8, 0, 0, 100, 0, 0) == VS_ERR_UNSUPPORTED);
  CHECK(CHK(&d, 4, 100, 4, 8, 0, 0, 100, 1, (size_t)1 << 31) == VS_ERR_UNSUPPORTED);
  vs_strack_opts b = d;
  b.max_reject = 0;
  CHECK(CHK(&b, 4, 100, 4, 8, 0, 0, 100, 0, 0) == VS_ERR_RANGE);
  b.max_reject = VS_ST_MAX_REJECT + 1;
  CHECK(CHK(&b, 4, 100, 4, 8, 0, 0, 100, 0, 0) == VS_ERR_RANGE);
  b.max_reject = VS_ST_MAX_REJECT;
  CHECK(CHK(&b, 4, 100, 4, 8, 0, 0, 100, 0, 0) == VS_OK && o.max_reject == VS_ST_MAX_REJECT);
  b.max_reject = 1;
  CHECK(CHK(&b, 4, 100, 4, 8, 0, 0, 100, 0, 0) == VS_OK);
  b.reserved_ = 1;
  b.max_reject = 0;
  CHECK(CHK(&b, 4, 100, 4, 8, 0, 0, 100, 0, 0) == VS_ERR_ARG);

  /* the row of the pitch track's frames */
  vs_strack_row r;
  vs_pitch_opts po;
  vs_pitch_defaults(&po);
  CHECK(vs_strack_from_pitch(NULL, 16000, 16000, NULL) == VS_ERR_ARG);
  CHECK(vs_strack_from_pitch(NULL, 16000, 16000, &r) == VS_OK);
  CHECK(r.n_frames == 94 && r.hop == 160 && r.offset == 480 - 80 && r.length == 16000 && r.pmin == 32 && r.pmax == 320);
  CHECK(vs_strack_from_pitch(&po, 16000, 962, &r) == VS_OK && r.n_frames == 1);
  CHECK(vs_strack_from_pitch(&po, 16000, 961, &r) == VS_ERR_RANGE && vs_strack_from_pitch(&po, 16000, 0, &r) == VS_ERR_RANGE);
  CHECK(vs_strack_from_pitch(&po, 999, 5000, &r) == VS_ERR_RANGE && vs_strack_from_pitch(&po, 16000, -1, &r) == VS_ERR_RANGE);
  CHECK(vs_strack_from_pitch(&po, 96000, 2147483647, &r) == VS_OK && r.pmax == 1920 && r.hop == 960);
  CHECK(r.offset == 2880 - 480 && r.n_frames == 1 + (2147483647 - 5762) / 960);
  po.f0_min = 70.0f;
  po.hop_s = 0.005;
  CHECK(vs_strack_from_pitch(&po, 16000, 4000, &r) == VS_OK && r.pmax == 229 && r.hop == 80);
  CHECK(r.offset == 229 + 114 - 40 && r.n_frames == 1 + (4000 - 689) / 80);
  po.jump_q = -1;
  CHECK(vs_strack_from_pitch(&po, 16000, 4000, &r) == VS_ERR_ARG);

  /* the plan: the refusals of every row, the T2 that are needed, the block */
  enum { ROWS = 5, NS = 4000, FP = 20 };
  vs_lane lanes[ROWS];
  vs_strack_row rows[ROWS], good[ROWS];
  for (int i = 0; i < ROWS; i++) {
    CHECK(vs_lane_defaults(&lanes[i]) == VS_OK);
    lanes[i].seed = 0x123456789abcdef0ull + (uint64_t)i;
    good[i] = (vs_strack_row){FP, 160, -2147483647 - 1, NS, 32, 320};
  }
  lanes[1].cq = 1.0f;
  lanes[1].flags = VS_FLAG_JITTER | VS_FLAG_SHIMMER | VS_FLAG_NOISE;
  lanes[1].jitter = 0.0f; /* the flag without a value: no jitter */
  lanes[1].shimmer = 0.05f;
  lanes[1].noise = 100.0f;
  lanes[1].DC = 70000.5f; /* (short)DC wraps */
  good[1] = (vs_strack_row){1, 2147483647, 2147483647, 0, 2, VS_AC_MAX_LAG};
  lanes[2].cq = 0.25f;
  good[2] = (vs_strack_row){3, 1, 0, NS - 1, 900, 901};
  good[4] = good[0];
  uint8_t need[VS_ST_T2_MAX + 1];
  VsStPlan plan;
#define BAD(i, field, value) (memcpy(rows, good, sizeof(rows)), rows[i].field = (value), vs_strack_plan(lanes, rows, ROWS, NS, FP, need, &plan))
  CHECK(BAD(0, n_frames, 0) == VS_ERR_RANGE && BAD(3, n_frames, FP + 1) == VS_ERR_RANGE && BAD(3, n_frames, FP) == VS_OK);
  CHECK(BAD(2, hop, 0) == VS_ERR_RANGE && BAD(2, hop, -5) == VS_ERR_RANGE);
  CHECK(BAD(4, length, -1) == VS_ERR_RANGE && BAD(4, length, NS + 1) == VS_ERR_RANGE && BAD(4, length, 0) == VS_OK);
  CHECK(BAD(0, pmin, 1) == VS_ERR_RANGE && BAD(0, pmax, VS_AC_MAX_LAG + 1) == VS_ERR_RANGE && BAD(0, pmin, 321) == VS_ERR_RANGE);
  CHECK(BAD(0, pmin, 320) == VS_OK && BAD(0, offset, 2147483647) == VS_OK);
  lanes[3].cq = 0.0f; /* vs_lane_validate's answer comes first */
  CHECK(BAD(3, hop, 0) == VS_ERR_UNSUPPORTED);
  lanes[3].cq = 0.6f;
  lanes[3].amp = 32767;
  CHECK(BAD(3, hop, 160) == VS_ERR_RANGE);
  lanes[3].amp = 12000;

  memcpy(rows, good, sizeof(rows));
  CHECK(vs_strack_plan(lanes, rows, ROWS, NS, FP, need, &plan) == VS_OK);
  size_t entries = 0;
  for (int t = 0; t <= VS_ST_T2_MAX; t++) {
    int want = 0;
    for (int i = 0; i < ROWS; i++) want |= t >= t2(lanes[i].cq, rows[i].pmin) && t <= t2(lanes[i].cq, rows[i].pmax);
    CHECK(need[t] == want);
    if (want) entries += (size_t)t;
  }
  CHECK(need[1] && need[1024] && !need[0] && !need[1025]); /* row 1: cq 1 over 2..2048 */
  CHECK(plan.toff_at == ROWS * 80 && plan.cos_at == ROWS * 80 + 4104 && plan.cos_entries == entries);
  CHECK(plan.bytes == plan.cos_at + entries * 8);
  /* rows whose stretches neither touch nor repeat: three separate runs of T2 */
  vs_strack_row apart[3] = {{1, 1, 0, 0, 100, 110}, {1, 1, 0, 0, 400, 410}, {1, 1, 0, 0, 100, 110}};
  lanes[2].cq = 0.5f;
  vs_lane three[3] = {lanes[2], lanes[2], lanes[2]};
  CHECK(vs_strack_plan(three, apart, 3, NS, FP, need, &plan) == VS_OK);
  for (int t = 0; t <= VS_ST_T2_MAX; t++) CHECK(need[t] == ((t >= 25 && t <= 28) || (t >= 100 && t <= 103)));
  lanes[2].cq = 0.25f;

  /* the launch: refusals before anything is staged, then the block and the arguments */
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(struct vs_ctx));
  int32_t *period = (int32_t *)calloc((size_t)ROWS * FP * 24, sizeof(int32_t)), *amp = (int32_t *)calloc((size_t)ROWS * FP, 4);
  int16_t *flow = (int16_t *)calloc((size_t)ROWS * (NS + 8), sizeof(int16_t));
  vs_strack_stat stat[ROWS];
  vs_strack_cycle *cyc = (vs_strack_cycle *)calloc((size_t)ROWS * 7, sizeof(vs_strack_cycle));
  CHECK(ctx && period && amp && flow && cyc);
  memcpy(rows, good, sizeof(rows));
#define LAUNCH(c, l, r, p, ps, a, as, f, op, s, cy, cp) \
  vs_strack_launch(c, &d, l, ROWS, NS, r, p, ps, FP, a, as, f, op, s, cy, cp)
  CHECK(LAUNCH(NULL, lanes, rows, period, 96, amp, 4, flow, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, NULL, rows, period, 96, amp, 4, flow, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, NULL, period, 96, amp, 4, flow, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, NULL, 96, amp, 4, flow, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, period, 96, amp, 4, NULL, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, period, 96, amp, 4, flow, NS + 8, NULL, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, period, 96, amp, 4, flow, NS + 8, stat, cyc, 0) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, period, 98, amp, 4, flow, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, period, 96, amp, 0, flow, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, period, 96, amp, 4, flow, NS - 1, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(LAUNCH(ctx, lanes, rows, (int32_t *)((char *)period + 2), 96, amp, 4, flow, NS + 8, stat, cyc, 7) == VS_ERR_ARG);
  rows[2].hop = 0;
  CHECK(LAUNCH(ctx, lanes, rows, period, 96, amp, 4, flow, NS + 8, stat, cyc, 7) == VS_ERR_RANGE);
  rows[2].hop = 1;
  CHECK(launches == 0 && !staged && blocks_out == 0);

  o = d;
  o.max_reject = 9;
  CHECK(vs_strack_launch(ctx, &o, lanes, ROWS, NS, rows, period + 3, 96, FP, amp, 8, flow, NS + 8, stat, cyc, 7) == VS_OK);
  CHECK(launches == 1 && blocks_out == 0);
  CHECK(vs_strack_plan(lanes, rows, ROWS, NS, FP, need, &plan) == VS_OK && seen_bytes == plan.bytes);
  CHECK((const char *)seen.period == (const char *)(period + 3) && seen.period_stride == 96 && seen.frames_pitch == FP);
  CHECK((const char *)seen.amp == (const char *)amp && seen.amp_stride == 8 && seen.out == flow && seen.out_pitch == NS + 8);
  CHECK(seen.stat == stat && seen.cycles == cyc && seen.cycles_pitch == 7 && seen.n_lanes == ROWS && seen.max_reject == 9);
  CHECK((const char *)seen.toff - (const char *)seen.rows == (long)plan.toff_at);
  CHECK((const char *)seen.costab - (const char *)seen.rows == (long)plan.cos_at);
  const VsStRow *sr = (const VsStRow *)seen_block;
  const int32_t *toff = (const int32_t *)((const char *)seen_block + plan.toff_at);
  const double *cosv = (const double *)((const char *)seen_block + plan.cos_at);
  for (int i = 0; i < ROWS; i++) {
    CHECK(sr[i].n_frames == rows[i].n_frames && sr[i].hop == rows[i].hop && sr[i].offset == rows[i].offset);
    CHECK(sr[i].length == rows[i].length && sr[i].pmin == rows[i].pmin && sr[i].pmax == rows[i].pmax);
    CHECK(sr[i].key0 == (uint32_t)lanes[i].seed && sr[i].key1 == (uint32_t)(lanes[i].seed >> 32) && sr[i].amp == lanes[i].amp);
    CHECK(sr[i].cq == lanes[i].cq && sr[i].K == lanes[i].K && sr[i].DC == lanes[i].DC && sr[i].noise == lanes[i].noise);
    CHECK(sr[i].reserved_[0] == 0 && sr[i].reserved_[1] == 0);
  }
  CHECK(sr[1].flags == (VS_STF_SHIMMER | VS_STF_NOISE) && sr[0].flags == 0 && sr[1].dcs == 70000 - 65536);
  size_t at = 0;
  for (int t = 0; t <= VS_ST_T2_MAX; t++) {
    if (!need[t]) {
      CHECK(toff[t] == -1);
      continue;
    }
    CHECK(toff[t] == (int32_t)at);
    CHECK(cosv[at] == 1.0 && (t < 2 || cosv[at + (size_t)t - 1] == cos(4.0 * atan(1.0) * (t - 1) / t)));
    at += (size_t)t;
  }
  CHECK(at == plan.cos_entries);
  /* without an amplitude track and a log */
  CHECK(vs_strack_launch(ctx, NULL, lanes, ROWS, NS, rows, period, 4, FP, NULL, 77, flow, NS, stat, NULL, 55) == VS_OK);
  CHECK(launches == 2 && seen.amp == NULL && seen.amp_stride == 0 && seen.cycles == NULL && seen.cycles_pitch == 0);
  CHECK(seen.max_reject == 256 && seen.period_stride == 4 && blocks_out == 0);

  /* the host-buffer call: the same refusals, the caller's arrays as the launch's */
  CHECK(vs_strack(ctx, &d, lanes, ROWS, NS, rows, NULL, FP, amp, flow, stat, cyc, 7) == VS_ERR_ARG);
  CHECK(vs_strack(ctx, &d, lanes, ROWS, NS, rows, period, FP, amp, flow, NULL, cyc, 7) == VS_ERR_ARG);
  CHECK(vs_strack(ctx, &d, lanes, ROWS, NS, rows, period, FP, amp, flow, stat, cyc, 0) == VS_ERR_ARG);
  rows[0].pmin = 1;
  CHECK(vs_strack(ctx, &d, lanes, ROWS, NS, rows, period, FP, amp, flow, stat, cyc, 7) == VS_ERR_RANGE);
  rows[0].pmin = 32;
  CHECK(launches == 2);
  CHECK(vs_strack(ctx, &d, lanes, ROWS, NS, rows, period, FP, amp, flow, stat, cyc, 7) == VS_OK && launches == 3);
  CHECK((const char *)seen.period == (const char *)period && seen.period_stride == 4 && (const char *)seen.amp == (const char *)amp);
  CHECK(seen.amp_stride == 4 && seen.out == flow && seen.out_pitch == NS && seen.stat == stat && seen.cycles == cyc);
  CHECK(vs_strack(ctx, NULL, lanes, ROWS, NS, rows, period, FP, NULL, flow, stat, NULL, 0) == VS_OK && launches == 4);
  CHECK(seen.amp == NULL && seen.cycles == NULL && blocks_out == 0);

  free(staged);
  free(seen_block);
  free(period);
  free(amp);
  free(flow);
  free(cyc);
  free(ctx);
  printf("ok\n");
  return 0;
}
