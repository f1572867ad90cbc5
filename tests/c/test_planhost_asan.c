/* The device-free half of plan creation (voice_synth_amd/csrc/vs_planhost.c) and the gather bookkeeping of
 * vs_host.c under AddressSanitizer + UBSan + the thread pool of the expansion.  Built and run by
 * tests/test_host_sanitizers.py:
 *   gcc -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tests/c/test_planhost_asan.c \
 *       voice_synth_amd/csrc/vs_planhost.c voice_synth_amd/csrc/vs_host.c -Iinclude -lm -lpthread
 * What it goes through: the expansion of 20000 lanes of mixed periods on 8 threads, the failure of the LOWEST bad
 * lane whatever the thread (and the order) that met it, the kernel order by (P, T2, options) found from the lanes and
 * written straight into place -- a permutation, sorted, ties in input order --, the mixed-rings table of a batch of many periods (every group once, every ring deep, every workgroup inside
 * the LDS), the launch shape, launch knobs and block layouts of plans from one lane to a full grid (vs_plan_shape,
 * vs_plan_knobs, vs_plan_layout: what fits the LDS, when three roles run, when the hardware is asked), the ring policy
 * over every period it can be asked for, the same over long periods (the narrow build: its ring, its cos rows, its
 * thresholds, and a refusal that is never the policy's whim), cos rows, the rounds of a node's gather; which kernel, block,
 * grid and LDS a launch gets (vs_launch_pick and its kin) against a copy of the launchers that used to decide it, over every selector. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../voice_synth_amd/csrc/vs_planhost.h"

int vs_shard_cut(size_t n_lanes, int n_shards, int shard, size_t *lo, size_t *hi);
size_t vs_gather_rounds(size_t n_lanes, int n_shards, size_t chunk);
int vs_gather_round(size_t n_lanes, int n_shards, int shard, size_t chunk, size_t round, size_t *row0, size_t *rows);

static int fails = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      fails++;                                                          \
    }                                                                   \
  } while (0)

static unsigned rng_state = 12345u;
static unsigned rnd(void)
{
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

/* a stand-in for the context's page-locked allocator: counts, and refuses the calls whose bit is set in big_refuse_mask */
static int big_calls = 0, big_live = 0;
static unsigned big_refuse_mask = 0;
static void *big_alloc_stub(void *user, size_t bytes)
{
  const int k = big_calls++;
  if (k < 32 && (big_refuse_mask >> k) & 1u) return NULL;
  if (k >= 32 && big_refuse_mask == ~0u) return NULL;
  char *p = (char *)malloc(bytes + 16);
  if (!p) return NULL;
  memcpy(p, "BIGALLOC", 8); /* a block of ours: free() of p + 16 would be caught by the sanitizer */
  (*(int *)user)++;
  return p + 16;
}
static void big_free_stub(void *user, void *ptr)
{
  char *p = (char *)ptr - 16;
  if (memcmp(p, "BIGALLOC", 8) != 0) abort();
  (*(int *)user)--;
  free(p);
}

/* a stand-in for the context's answer to "are the wavefronts dealt four at a time?" */
static int dealt_calls = 0, dealt_answer = 1, dealt_waves = 0;
static int dealt_stub(void *user, int waves)
{
  (void)user;
  dealt_calls++;
  dealt_waves = waves;
  return dealt_answer;
}

/* ---- the launchers of csrc/vs_kernels.hip as they stood before their decisions moved to vs_planhost.c ----
 * Copied from csrc/vs_kernels.hip at commit d62cd9a: vs_pick_log, vs_pick_ws2, vs_pick_ws and the body of VS_LAUNCH_NAME
 * (the section "launch table", lines 1376-1458), and the geometry lines of vs_launch_out_noise (lines 1012-1033).  What
 * had to change for a C program without a device: a function pointer is the identifier of the kernel it pointed to
 * (vs_pick_log<A, K, P>(log) stood for vs_synth_kernel<A, K, log, P>); the two builds of the file (#if VS_GROUP_LANES ==
 * VS_WAVE) are the parameter `narrow`, VS_ONOISE_ROWMAJOR and VS_ONOISE_OCTETS parameters too; hipErrorInvalidValue is
 * refused = 1, and the launch is the values it was given.  One line could not be taken over: with ws_pairs == 0 the
 * launcher divided the grid by zero (no plan makes such a launch); the copy says so (div0) and the selection must refuse. */
typedef struct Was {
  int refused, div0, fn;
  unsigned block, grid;
  size_t lds_bytes;
} Was;
#define WAS_PICK_LOG(ARITH, KIND, PRE1, log) VS_KERNEL_ID(narrow ? VS_KF_NARROW : VS_KF_ONE_WAVE, ARITH, KIND, (log) ? 1 : 0, PRE1)
static int was_pick_ws2(int ARITH, int PRE1, bool three, bool pow)
{
  if (three) return pow ? VS_KERNEL_ID(VS_KF_WS_POW, ARITH, PRE1, 3, 0) : VS_KERNEL_ID(VS_KF_WS, ARITH, PRE1, 3, 0);
  return pow ? VS_KERNEL_ID(VS_KF_WS_POW, ARITH, PRE1, 2, 0) : VS_KERNEL_ID(VS_KF_WS, ARITH, PRE1, 2, 0);
}
static int was_pick_ws(int arith, bool pre1, bool three, bool pow)
{
  if (arith == VS_ARITH_EXACT) return pre1 ? was_pick_ws2(VS_ARITH_EXACT, 1, three, pow) : was_pick_ws2(VS_ARITH_EXACT, 0, three, pow);
  if (arith == VS_ARITH_F32) return pre1 ? was_pick_ws2(VS_ARITH_F32, 1, three, pow) : was_pick_ws2(VS_ARITH_F32, 0, three, pow);
  return pre1 ? was_pick_ws2(VS_ARITH_FMA, 1, three, pow) : was_pick_ws2(VS_ARITH_FMA, 0, three, pow);
}
static Was was_launch(bool narrow, int arith, int kind, bool log, bool wave_specialised, bool pre1, const VsKernelArgs *args,
                      unsigned grid, size_t lds_bytes)
{
  Was w = {0, 0, 0, 0, 0, 0};
  int fn = 0;
  unsigned block = VS_WAVE;
  if (!narrow) { /* #if VS_GROUP_LANES == VS_WAVE */
    if (args->group_lanes != 0 && args->group_lanes != VS_WAVE) {
      /* periods beyond the 64-column ring: the narrow build of this file (16 utterances per wavefront) */
      return was_launch(true, arith, kind, log, false, pre1, args, grid, lds_bytes); /* vs_launch_kernel_narrow */
    }
    if (wave_specialised && kind == VS_KIND_SYNTH && !log) {
      const bool three = args->ws_roles == 3;
      const bool pow = args->ondw && args->odone && args->pow_lframe > 0;
      fn = was_pick_ws(arith, pre1, three, pow);
      block = (unsigned)args->ws_roles * VS_WAVE * (unsigned)args->ws_pairs;
      if (three && args->ws_layout == VS_WS_LAYOUT_SPREAD_2X3) {
        if (args->ws_pairs != 2) return w.refused = 1, w;
        block = 8 * VS_WAVE;
      }
      if (!args->group_map) lds_bytes = (size_t)args->ws_pair_bytes * (size_t)args->ws_pairs;
      else if (args->ws_pairs != 4 || (three && args->ws_layout != VS_WS_LAYOUT_ROLE_MAJOR)) return w.refused = 1, w;
      if (args->ws_pairs == 0) return w.div0 = 1, w; /* (not in the original: the next line divides by it) */
      grid = (grid + (unsigned)args->ws_pairs - 1) / (unsigned)args->ws_pairs;
    }
  } /* #endif */
  if (!fn) { /* the one-wave kernel */
    if (arith == VS_ARITH_F32) arith = VS_ARITH_FMA;
    if (arith == VS_ARITH_EXACT) {
      if (kind == VS_KIND_SYNTH) fn = pre1 ? WAS_PICK_LOG(VS_ARITH_EXACT, VS_KIND_SYNTH, 1, log) : WAS_PICK_LOG(VS_ARITH_EXACT, VS_KIND_SYNTH, 0, log);
      else if (kind == VS_KIND_SOURCE) fn = WAS_PICK_LOG(VS_ARITH_EXACT, VS_KIND_SOURCE, 0, log);
      else if (kind == VS_KIND_FILTER) fn = pre1 ? WAS_PICK_LOG(VS_ARITH_EXACT, VS_KIND_FILTER, 1, false) : WAS_PICK_LOG(VS_ARITH_EXACT, VS_KIND_FILTER, 0, false);
    } else if (arith == VS_ARITH_FMA) {
      if (kind == VS_KIND_SYNTH) fn = WAS_PICK_LOG(VS_ARITH_FMA, VS_KIND_SYNTH, 0, log);
      else if (kind == VS_KIND_SOURCE) fn = WAS_PICK_LOG(VS_ARITH_EXACT, VS_KIND_SOURCE, 0, log);
      else if (kind == VS_KIND_FILTER) fn = WAS_PICK_LOG(VS_ARITH_FMA, VS_KIND_FILTER, 0, false);
    }
  }
  if (!fn) return w.refused = 1, w;
  if (kind == VS_KIND_FILTER) lds_bytes = 0;
  w.fn = fn;
  w.grid = grid;
  w.block = block;
  w.lds_bytes = lds_bytes;
  return w;
}

typedef struct WasNoise {
  int refused, fill, vec;
  long pblocks, segs;
  unsigned grid_x, grid_y, seg_magic, seg_shift, fgrid;
} WasNoise;
static WasNoise was_out_noise(const VsKernelArgs *args, int VS_ONOISE_OCTETS, int VS_ONOISE_ROWMAJOR)
{
  WasNoise w;
  memset(&w, 0, sizeof(w));
  if (!args->ondw || args->ondw_pitch <= 0) return w.refused = 1, w;
  const long frames = (long)args->n_lanes * args->ondw_pitch;
  const long pblocks = (frames + 255) / 256;
  const long per_block = 2048L * VS_ONOISE_OCTETS; /* 256 threads x 8 samples x octets */
  const long segs = ((long)args->n_samples + per_block - 1) / per_block;
  if (pblocks > 0x7FFFFFFFL) return w.refused = 1, w;
  unsigned seg_magic = 0, seg_shift = 0;
  if (VS_ONOISE_ROWMAJOR) {
    const long nblocks = segs * (long)args->n_lanes;
    if (nblocks > 0x7FFFFFFFL) return w.refused = 1, w;
    unsigned k = 0;
    while ((1ull << k) < (unsigned long long)segs) k++;
    seg_magic = segs > 1 ? (unsigned)(((1ull << (31 + k)) / (unsigned long long)segs) + 1ull) : 0u;
    seg_shift = segs > 1 ? k - 1 : 0u;
    w.grid_x = (unsigned)nblocks;
    w.grid_y = 1;
  } else {
    if (segs > 65535L) return w.refused = 1, w;
    w.grid_x = (unsigned)args->n_lanes;
    w.grid_y = (unsigned)segs;
  }
  w.fill = args->odone != NULL; /* the fused kernel took the frame powers along */
  w.fgrid = (unsigned)((args->n_lanes + 63) / 64);
  w.vec = args->vec_ok ? 1 : 0;
  w.pblocks = pblocks;
  w.segs = segs;
  w.seg_magic = seg_magic;
  w.seg_shift = seg_shift;
  return w;
}

/* the noise pass as the selection and the copy see it, and the kernel's own division of a block by segs */
static void check_out_noise(const VsKernelArgs *a, int octets, int row_major)
{
  VsOutNoisePick p;
  const WasNoise w = was_out_noise(a, octets, row_major);
  const int rc = vs_launch_pick_out_noise(a, octets, row_major, &p);
  CHECK((rc != 0) == w.refused);
  if (rc != 0 || w.refused) return;
  CHECK(p.power.kernel == VS_KERNEL_ID(w.fill ? VS_KF_OUT_POWER_FILL : VS_KF_OUT_POWER, w.vec, 0, 0, 0));
  CHECK(p.power.grid == (w.fill ? w.fgrid : (unsigned)w.pblocks) && p.power.block == (w.fill ? 64u : 256u) && p.power.lds_bytes == 0);
  CHECK(p.noise.kernel == VS_KERNEL_ID(VS_KF_OUT_NOISE, w.vec, 0, 0, 0) && p.noise.block == 256 && p.noise.lds_bytes == 0);
  CHECK(p.noise.grid == w.grid_x && p.noise_grid_y == w.grid_y);
  CHECK(p.segs == (unsigned)w.segs && p.seg_magic == w.seg_magic && p.seg_shift == w.seg_shift);
  if (!row_major) return;
  const uint64_t segs = p.segs, nblocks = p.noise.grid;
  if (segs == 1) {
    CHECK(p.seg_magic == 0); /* the kernel takes the block itself */
    return;
  }
  int bad = 0;
  for (int k = 0; k < 1004 && nblocks; k++) {
    uint64_t block = k == 0 ? 0 : k == 1 ? segs - 1 : k == 2 ? segs : k == 3 ? nblocks - 1 : (((uint64_t)rnd() << 24) ^ rnd()) % nblocks;
    if (block >= nblocks) block = nblocks - 1;
    bad += (unsigned)(((unsigned long long)(unsigned)block * p.seg_magic) >> 32) >> p.seg_shift != (unsigned)(block / segs);
  }
  CHECK(bad == 0);
}

/* ---- long periods: the batches of the second shape loop (the narrow build, tests/test_narrow_ref.py) ---- */
/* a lane with source options of its own near the shortest periods that make a plan narrow: 48 .. 64 kHz, F0 50 .. 55 Hz, cq
 * 0.30 .. 0.89, 3 % jitter on three lanes of four, shimmer and glottal noise mixed */
static void long_lane(vs_lane *l, size_t i)
{
  static const int rates[4] = {64000, 56000, 48000, 50000};
  vs_lane_defaults(l);
  l->fs = rates[i % 4];
  l->F0 = 50.0f + 5.0f * (float)((7 * i) % 1013) / 1012.0f;
  l->Fg = l->F0 * 125.0f / 120.0f + 1.0f;
  l->cq = 0.30f + 0.59f * (float)((13 * i) % 1021) / 1020.0f; /* (a cos row of its own for nearly every lane of a big batch too) */
  if (i % 4 != 3) {
    l->flags |= VS_FLAG_JITTER;
    l->jitter = 0.03f;
  }
  if (i % 3) {
    l->flags |= VS_FLAG_SHIMMER;
    l->shimmer = 0.02f + 0.005f * (float)(i % 33);
  }
  if (i & 1) {
    l->flags |= VS_FLAG_NOISE;
    l->noise = 100.0f;
    l->DC = 0.25f;
  }
  l->vowel = "12467"[i % 5];
  l->seed = 1 + i;
}
/* 16000 and 22050 Hz, F0 100 .. 250: periods of 64 .. 220 samples */
static void short_lane(vs_lane *l, size_t i)
{
  vs_lane_defaults(l);
  l->fs = (i & 1) ? 22050 : 16000;
  l->F0 = 100.0f + (float)((11 * i) % 151);
  l->Fg = l->F0 * 125.0f / 120.0f + 1.0f;
  if (i % 3) {
    l->flags |= VS_FLAG_JITTER | VS_FLAG_SHIMMER | VS_FLAG_NOISE;
    l->jitter = 0.01f;
    l->shimmer = 0.0576f;
    l->noise = 100.0f;
    l->DC = 0.25f;
  }
  l->seed = 1 + i;
}
/* The batch a plan refuses although each of its lanes passes alone (tests/test_narrow_ref.py, REFUSED, has the same lanes):
 * periods near the top of the narrow build's range and a cos row of its own per lane; everything else vs_lane_defaults' */
#define N_REFUSED 15
static const struct { int fs; float F0, Fg, cq; } refused_spec[N_REFUSED] = {
    {176400, 50.0f, 52.0f, 0.30f}, {176400, 56.0f, 58.0f, 0.35f}, {176400, 64.0f, 66.0f, 0.42f}, {176400, 79.0f, 81.0f, 0.45f},
    {96000, 50.0f, 52.0f, 0.55f},  {96000, 52.0f, 54.0f, 0.60f},  {96000, 55.0f, 57.0f, 0.65f},  {96000, 60.0f, 62.0f, 0.70f},
    {88200, 50.0f, 52.0f, 0.75f},  {88200, 53.0f, 55.0f, 0.80f},  {88200, 58.0f, 60.0f, 0.85f},  {88200, 66.0f, 68.0f, 0.89f},
    {44100, 50.0f, 52.0f, 0.85f},  {44100, 51.0f, 53.0f, 0.89f},  {44100, 79.0f, 81.0f, 0.80f}};
static void refused_lane(vs_lane *l, size_t i)
{
  vs_lane_defaults(l);
  l->fs = refused_spec[i].fs;
  l->F0 = refused_spec[i].F0;
  l->Fg = refused_spec[i].Fg;
  l->cq = refused_spec[i].cq;
  l->seed = 900 + i;
}
enum { LB_HOM, LB_HET, LB_SHORT_LONG, LB_REFUSED, LB_REFUSED_ALONE, LB_KINDS };
static void long_batch(int kind, vs_lane *l, size_t m, size_t pick)
{
  for (size_t i = 0; i < m; i++) {
    if (kind == LB_HOM) {
      long_lane(&l[i], 0);
      l[i].seed = 1 + i;
    } else if (kind == LB_HET) {
      long_lane(&l[i], i);
    } else if (kind == LB_SHORT_LONG) {
      if (i % 16 == 5 || m == 1) long_lane(&l[i], 4 * (i / 16));
      else short_lane(&l[i], i);
    } else {
      refused_lane(&l[i], kind == LB_REFUSED ? i : pick);
    }
  }
}
/* what a plan of these records needs of the LDS at the least, worked out here: the smallest ring that takes the batch's
 * longest cycle (a super-step, the cycle, the trash rows, up to a multiple of the super-step; 16 columns of int16) and the
 * cos rows of the worst wavefront of 16 -- (T2 + 7) & ~7 doubles for every distinct T2 among its lanes */
static size_t narrow_need(const VsDevLane *rec, size_t m, int *ring, int *worst_rows)
{
  int tmax = 1, worst = 0;
  for (size_t w0 = 0; w0 < m; w0 += VS_NARROW_LANES) {
    int seen[VS_NARROW_LANES], ns = 0, sum = 0;
    for (size_t l = w0; l < m && l < w0 + VS_NARROW_LANES; l++) {
      if (rec[l].tbound > tmax) tmax = rec[l].tbound;
      int dup = 0;
      for (int q = 0; q < ns; q++) dup |= seen[q] == rec[l].T2;
      if (!dup) {
        seen[ns++] = rec[l].T2;
        sum += (rec[l].T2 + 7) & ~7;
      }
    }
    if (sum > worst) worst = sum;
  }
  *ring = (VS_SS + tmax + VS_TRASH_ROWS + VS_SS - 1) / VS_SS * VS_SS;
  *worst_rows = worst;
  return (size_t)(*ring + VS_TRASH_ROWS) * VS_NARROW_LANES * sizeof(int16_t) + (size_t)worst * sizeof(double);
}

int main(void)
{
  const size_t n = 20000;
  vs_lane *lanes = (vs_lane *)malloc(n * sizeof(vs_lane));
  VsDevLane *dl = (VsDevLane *)malloc(n * sizeof(VsDevLane));
  CHECK(lanes && dl);
  for (size_t l = 0; l < n; l++) {
    CHECK(vs_lane_defaults(&lanes[l]) == VS_OK);
    lanes[l].fs = 16000;
    lanes[l].F0 = 80.0f + (float)(rnd() % 221);         /* periods 53..200: many distinct (P, T2) */
    lanes[l].Fg = lanes[l].F0 * 125.0f / 120.0f + 1.0f;
    lanes[l].jitter = 0.01f;
    lanes[l].shimmer = 0.0576f;
    lanes[l].noise = 100.0f;
    lanes[l].DC = 0.25f;
    lanes[l].flags = (rnd() & 1) ? (VS_FLAG_JITTER | VS_FLAG_SHIMMER | VS_FLAG_NOISE) : VS_FLAG_JITTER;
    lanes[l].vowel = "12467"[l % 5];
    lanes[l].seed = 1 + l;
  }
  CHECK(vs_expand_all(lanes, dl, n, 0) == VS_OK);
  for (size_t l = 0; l < n; l++) CHECK(dl[l].row == (int32_t)l && dl[l].P == (int)((float)lanes[l].fs / lanes[l].F0));
  {
    /* the batch's statistics, gathered by the threads that make the records, against a walk over the records */
    VsBatchStats st, st2;
    lanes[11].pre_emphasis = 0.5f;
    lanes[12].out_snr = 100.0f;
    CHECK(vs_expand_all_stats(lanes, dl, n, 0, &st) == VS_OK);
    int max_T2 = 0, tmax = 1, minlf = 0, pre1 = 1;
    size_t noisy = 0;
    for (size_t l = 0; l < n; l++) {
      if (dl[l].T2 > max_T2) max_T2 = dl[l].T2;
      if (dl[l].tbound > tmax) tmax = dl[l].tbound;
      if (dl[l].Lframe > 0 && (minlf == 0 || dl[l].Lframe < minlf)) minlf = dl[l].Lframe;
      if (dl[l].pre != 1.0) pre1 = 0;
      if (dl[l].flags & VS_DF_NOISE) noisy++;
    }
    CHECK(st.max_T2 == max_T2 && st.tmax == tmax && st.min_lframe == minlf && st.pre1 == pre1 && pre1 == 0);
    CHECK(st.n_noisy == noisy && st.any_onoise == 1 && st.wide == 0);
    VsDevLane *tmp = (VsDevLane *)malloc(n * sizeof(VsDevLane));
    CHECK(vs_expand_all_ordered(lanes, tmp, n, NULL, &st2) == VS_OK);
    CHECK(memcmp(&st, &st2, sizeof(st)) == 0);       /* the same batch in the kernels' order */
    free(tmp);
    lanes[11].pre_emphasis = 1.0f;
    lanes[12].out_snr = 0.0f;
    CHECK(vs_expand_all_stats(lanes, dl, n, 0, &st) == VS_OK && st.pre1 == 1 && st.any_onoise == 0);
  }

  /* the order: the records of vs_expand_all_ordered are a permutation of vs_expand_all's, sorted by (P, T2, options),
   * ties in input order; vs_kernel_order says the same */
  VsDevLane *sorted = (VsDevLane *)malloc(n * sizeof(VsDevLane));
  int reordered = 0;
  CHECK(vs_expand_all_ordered(lanes, sorted, n, &reordered, NULL) == VS_OK && reordered == 1);
  uint32_t *order = NULL;
  CHECK(vs_kernel_order(lanes, n, &order) == VS_OK && order != NULL);
  unsigned char *seen = (unsigned char *)calloc(n, 1);
  for (size_t l = 0; l < n; l++) {
    CHECK(sorted[l].row >= 0 && (size_t)sorted[l].row < n);
    if (sorted[l].row >= 0 && (size_t)sorted[l].row < n) {
      CHECK(!seen[sorted[l].row]);
      seen[sorted[l].row] = 1;
      CHECK(memcmp(&sorted[l], &dl[sorted[l].row], sizeof(VsDevLane)) == 0);
      CHECK(order && order[l] == (uint32_t)sorted[l].row);
    }
    if (l > 0) {
      const VsDevLane *a = &sorted[l - 1], *b = &sorted[l];
      const unsigned fa = a->flags & 7u, fb = b->flags & 7u; /* jitter / shimmer / noise on: the option bits of the key */
      const int lt = (a->P != b->P) ? (a->P < b->P) : (a->T2 != b->T2) ? (a->T2 < b->T2) : (fa < fb);
      const int eq = a->P == b->P && a->T2 == b->T2 && fa == fb;
      CHECK(lt || eq);
      if (eq) CHECK(a->row < b->row);
    }
  }
  free(order);
  free(seen);
  /* mixed rings over the sorted records (313 groups, the last one ragged): every group exactly once, every ring deep
   * enough for ITS periods and a multiple of the super-step, every workgroup inside the LDS, regions back to back;
   * batches of 1 .. 9 groups; a floor no workgroup can afford is refused and leaves nothing behind */
  for (int pass = 0; pass < 12; pass++) {
    const size_t m = pass == 0 ? n : (pass == 1 ? 64 : (pass == 2 ? 65 : (size_t)(64 * pass - 17)));
    const int floor_slots = (pass & 1) ? 144 : 192;
    VsGroupSlot *gm = NULL;
    size_t n_wg = 0, lds = 0;
    int c_min = 0, c_max = 0;
    const int rc = vs_mixed_rings_build(sorted, m, floor_slots, &gm, &n_wg, &lds, &c_min, &c_max);
    CHECK(rc == VS_OK);
    if (rc != VS_OK) continue;
    const size_t n_groups = (m + 63) / 64;
    CHECK(n_wg == (n_groups + 3) / 4 && lds <= VS_LDS_LIMIT && c_min >= floor_slots && c_max >= c_min);
    unsigned char *hit = (unsigned char *)calloc(n_groups, 1);
    for (size_t w = 0; w < n_wg; w++) {
      size_t off = 0;
      for (int k = 0; k < 4; k++) {
        const VsGroupSlot *gs = &gm[w * 4 + k];
        if (gs->group < 0) continue;
        CHECK((size_t)gs->group < n_groups && !hit[gs->group]);
        hit[gs->group] = 1;
        int tb = 1, need_ltab = 0, seen_t2[64], ns = 0;
        for (size_t l = (size_t)gs->group * 64; l < m && l < ((size_t)gs->group + 1) * 64; l++) {
          if (sorted[l].tbound > tb) tb = sorted[l].tbound;
          int dup = 0;
          for (int q = 0; q < ns; q++) dup |= seen_t2[q] == sorted[l].T2;
          if (!dup) {
            seen_t2[ns++] = sorted[l].T2;
            need_ltab += (sorted[l].T2 + 7) & ~7;
          }
        }
        CHECK(gs->ring_slots % VS_SS == 0 && gs->ring_slots >= VS_SS + tb + VS_TRASH_ROWS && gs->ring_slots >= floor_slots);
        CHECK((double)(gs->ring_slots - VS_SS) / (double)tb >= 1.65);
        CHECK(gs->ltab_entries == need_ltab && (gs->lds_off & 15) == 0 && (size_t)gs->lds_off == off);
        off += (((size_t)(gs->ring_slots + VS_TRASH_ROWS) * 128 + (size_t)gs->ltab_entries * 8 + VS_SYNC_WORDS_3 * 64 * 4) + 15) & ~(size_t)15;
      }
      CHECK(off <= VS_LDS_LIMIT && off <= lds);
    }
    for (size_t g = 0; g < n_groups; g++) CHECK(hit[g]);
    free(hit);
    free(gm);
  }
  {
    VsGroupSlot *gm = (VsGroupSlot *)0x1;
    size_t n_wg = 7, lds = 7;
    int c_min = 7, c_max = 7;
    CHECK(vs_mixed_rings_build(sorted, n, 1200, &gm, &n_wg, &lds, &c_min, &c_max) == VS_ERR_UNSUPPORTED);
    CHECK(gm == (VsGroupSlot *)0x1 && n_wg == 7);
    CHECK(vs_mixed_rings_build(sorted, 0, 192, &gm, &n_wg, &lds, &c_min, &c_max) == VS_ERR_ARG);
  }
  free(sorted);
  /* small batches, and a homogeneous one: input order, no index array */
  for (size_t m = 1; m <= 70; m++) {
    VsDevLane *s2 = (VsDevLane *)malloc(m * sizeof(VsDevLane));
    CHECK(vs_expand_all_ordered(lanes + 100, s2, m, NULL, NULL) == VS_OK);
    for (size_t l = 1; l < m; l++) CHECK(s2[l - 1].P <= s2[l].P);
    free(s2);
  }
  {
    vs_lane same[40];
    VsDevLane out[40];
    uint32_t *ord = (uint32_t *)0x1;
    for (int i = 0; i < 40; i++) {
      same[i] = lanes[7];
      same[i].seed = 100 + (uint64_t)i;
    }
    int re = 1;
    CHECK(vs_kernel_order(same, 40, &ord) == VS_OK && ord == NULL);
    CHECK(vs_expand_all_ordered(same, out, 40, &re, NULL) == VS_OK && re == 0);
    for (int i = 0; i < 40; i++) CHECK(out[i].row == i && out[i].key0 == (uint32_t)(100 + i));
  }

  /* ONE workspace over batches of growing and shrinking size (what a context does: chunks of 16384 lanes, then a
   * whole batch): every answer equals the one-shot function's, whichever buffers the workspace already holds */
  {
    VsPlanWs *ws = vs_planws_create();
    CHECK(ws != NULL);
    const size_t sizes[] = {300, 9000, 64, 20000, 8192, 1, 20000};
    VsDevLane *want = (VsDevLane *)malloc(n * sizeof(VsDevLane));
    CHECK(want != NULL);
    for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); k++) {
      const size_t m = sizes[k];
      VsDevLane *got = NULL;
      VsBatchStats sa, sb;
      int ra = -1, rb = -1;
      CHECK(vs_expand_all_ordered_ws(ws, lanes, m, 0, &got, &ra, &sa) == VS_OK && got != NULL);
      CHECK(vs_expand_all_ordered(lanes, want, m, &rb, &sb) == VS_OK);
      CHECK(ra == rb && memcmp(&sa, &sb, sizeof(sa)) == 0);
      if (got) CHECK(memcmp(got, want, m * sizeof(VsDevLane)) == 0);
      CHECK(vs_expand_all_ordered_ws(ws, lanes, m, 1, &got, &ra, NULL) == VS_OK && ra == 0); /* filter-only: input order */
      CHECK(vs_expand_all(lanes, want, m, 1) == VS_OK);
      if (got) CHECK(memcmp(got, want, m * sizeof(VsDevLane)) == 0);
    }
    VsDevLane *got = NULL;
    CHECK(vs_expand_all_ordered_ws(ws, lanes, 0, 0, &got, NULL, NULL) == VS_ERR_ARG);
    CHECK(vs_expand_all_ordered_ws(NULL, lanes, 5, 0, &got, NULL, NULL) == VS_ERR_ARG);
    free(want);
    vs_planws_destroy(ws);
    vs_planws_destroy(NULL);
  }

  /* the workspace under page-locked-memory pressure: the context's allocator for big record buffers (hipHostMalloc there,
   * a counting stand-in here) refuses its first, its second, or every request -- a batch whose lanes must be put in
   * kernel order needs TWO buffers, and either may end up in ordinary memory; the answer is the same and every block goes
   * back to where it came from */
  {
    for (int refuse = 0; refuse < 4; refuse++) {
      big_calls = big_live = 0;
      big_refuse_mask = (refuse == 3) ? ~0u : (1u << refuse);
      VsPlanWs *ws = vs_planws_create();
      CHECK(ws != NULL);
      vs_planws_set_big_allocator(ws, big_alloc_stub, big_free_stub, &big_live);
      VsDevLane *want = (VsDevLane *)malloc(n * sizeof(VsDevLane));
      CHECK(want != NULL);
      for (int round = 0; round < 2; round++) {
        VsDevLane *got = NULL;
        int ra = -1, rb = -1;
        CHECK(vs_expand_all_ordered_ws(ws, lanes, n, 0, &got, &ra, NULL) == VS_OK && got != NULL && ra == 1);
        CHECK(vs_expand_all_ordered(lanes, want, n, &rb, NULL) == VS_OK && rb == 1);
        if (got) CHECK(memcmp(got, want, n * sizeof(VsDevLane)) == 0);
      }
      CHECK(big_calls >= 2);             /* both buffers were asked of the big allocator ... */
      free(want);
      vs_planws_destroy(ws);
      CHECK(big_live == 0);              /* ... and what it gave has been given back to it, nothing of it to free() */
    }
  }

  /* the launch shape and the knobs of a launch, over batch sizes from one lane to a full grid, two chip sizes, the tuning's
   * shape knobs and both answers of the hardware: what fits the LDS, when three roles may run, which thresholds the
   * records get, when the hardware is asked */
  {
    const size_t sizes[] = {1, 64, 300, 1100, 2100, 20000};
    const vs_tuning tunes[] = {{0}, {.ws_roles = 2}, {.ws_roles = 3}, {.kernel = VS_KERNEL_SINGLE}, {.ws_pairs = 1},
                               {.ws_pairs = 2}, {.ws_pairs = 4}, {.mixed_rings = -1}, {.ring_slots = 600},
                               {.fault = VS_FAULT_SIMD_DEALING}, {.mixed_rings = -1, .ws_roles = 3}};
    VsDevLane *rec = (VsDevLane *)malloc(n * sizeof(VsDevLane));
    CHECK(rec != NULL);
    for (size_t si = 0; si < sizeof(sizes) / sizeof(sizes[0]); si++) {
      const size_t m = sizes[si];
      for (int hom = 0; hom <= 1; hom++) { /* the batch of many periods, and m copies of one lane */
        vs_lane *src = lanes;
        if (hom) {
          src = (vs_lane *)malloc(m * sizeof(vs_lane));
          CHECK(src != NULL);
          for (size_t l = 0; l < m; l++) src[l] = lanes[3];
        }
        VsBatchStats st;
        VsPlanTables tab;
        CHECK(vs_expand_all_ordered(src, rec, m, NULL, &st) == VS_OK);
        CHECK(vs_plan_tables_build(src, rec, m, &st, 0, &tab) == VS_OK && tab.taps_off == (size_t)rec[m - 1].tab_off + (size_t)rec[m - 1].T2 + 1);
        for (size_t ti = 0; ti < sizeof(tunes) / sizeof(tunes[0]); ti++)
          for (int cus = 8; cus <= 256; cus += 248)
            for (int answer = 0; answer <= 1; answer++) {
              const vs_tuning *t = &tunes[ti];
              VsPlanShape sh;
              dealt_calls = 0;
              dealt_answer = answer;
              const int rc = vs_plan_shape(rec, m, 16000, &st, 0, cus, t, tab.ltab_entries, dealt_stub, NULL, &sh);
              CHECK(rc == VS_OK);
              if (rc == VS_OK) {
                const int mixed = sh.n_wg_mixed != 0;
                CHECK((sh.gmap != NULL) == mixed && sh.lds_bytes <= VS_LDS_LIMIT && sh.lds_one_wave <= VS_LDS_LIMIT);
                CHECK(sh.grid == (m + 63) / 64 && sh.group_lanes == VS_WAVE && sh.ring_slots % VS_SS == 0);
                if (sh.wave_specialised) CHECK((size_t)sh.ws_pairs * (size_t)sh.ws_pair_bytes <= VS_LDS_LIMIT);
                if (sh.wave_specialised) CHECK(sh.ws_pairs == 1 || sh.ws_pairs == 2 || sh.ws_pairs == 4);
                CHECK(sh.ws_roles == 2 || (sh.ws_roles == 3 && sh.wave_specialised));
                int all64 = 1;
                for (size_t l = 0; l < m; l++) {
                  const int thr = rec[l].ready_min;
                  CHECK(thr == 0 || thr == 32 || thr == 40 || thr == 48 || thr == 58 || thr == 64);
                  CHECK(thr == rec[l - l % 64].ready_min); /* one threshold per group */
                  all64 &= thr == 64;
                }
                /* three roles only over deep rings (every filter wavefront waits for all of its lanes), or when forced */
                if (sh.ws_roles == 3 && t->ws_roles != 3) CHECK(all64);
                if (mixed) CHECK(all64 && sh.ws_pairs == 4 && sh.wave_specialised && sh.ring_slots_min <= sh.ring_slots);
                if (t->ws_roles == 2) CHECK(sh.ws_roles == 2 && dealt_calls == 0);
                /* the hardware is asked once, by plans that end with several groups of three roles -- or fell back */
                const int asked = sh.wave_specialised && sh.ws_pairs > 1 && (sh.ws_roles == 3 || sh.simd_fallback) && t->fault != VS_FAULT_SIMD_DEALING;
                CHECK(dealt_calls == asked);
                if (sh.ws_pairs == 1 || !sh.wave_specialised) CHECK(dealt_calls == 0 && !sh.simd_fallback);
                if (asked) CHECK(dealt_waves == (sh.ws_pairs == 4 ? 12 : 8) && sh.simd_fallback == !answer);
                if (sh.simd_fallback) CHECK(sh.ws_roles == 2);
                CHECK(sh.ws_layout == (sh.ws_roles == 3 && sh.ws_pairs == 2 ? VS_WS_LAYOUT_SPREAD_2X3 : VS_WS_LAYOUT_ROLE_MAJOR));
                for (int arith = VS_ARITH_EXACT; arith <= VS_ARITH_F32; arith++) {
                  VsLaunchKnobs k;
                  vs_plan_knobs(&sh, t, arith, &k);
                  CHECK(k.ready_min >= 0 && k.ready_min <= 64 && k.gen_min >= 1 && k.gen_min <= 64 && k.gen_low >= VS_SS);
                  CHECK(k.spin_limit == 1 << 22 && k.ws_filter_prio == 3);
                  CHECK(k.ready_min == (sh.wave_specialised && !sh.ws_shared_simd && arith != VS_ARITH_EXACT ? 40 : 0));
                }
                VsPlanLayout lay;
                vs_plan_layout(m, tab.costab_len, &sh, &lay);
                CHECK(lay.small_bytes >= VS_SMALL_BLOCK_MIN && lay.small_off_err + 64 <= lay.small_bytes && lay.small_off_err % 64 == 0);
                CHECK(lay.small_off_gmap >= lay.cos_bytes + 8 && lay.small_off_err >= lay.small_off_gmap + lay.gmap_bytes);
                CHECK(lay.zc_off_cos >= lay.lanes_bytes && lay.zc_off_err >= lay.zc_off_cos + lay.cos_bytes + 8 && lay.zc_off_wide == lay.zc_off_err + 64);
                CHECK(lay.gmap_bytes == sh.n_wg_mixed * 4 * sizeof(VsGroupSlot) && lay.wide_bytes == 0 && lay.zc_bytes == lay.zc_off_wide + 64);
              }
              free(sh.gmap);
            }
        vs_plan_tables_release(&tab);
        CHECK(tab.costab == NULL);
        if (hom) free(src);
      }
    }
    free(rec);
  }

  /* the same over long periods: homogeneous and heterogeneous batches beyond the 64-column ring, short lanes with one long
   * lane in every 16, and the batch that is refused although each of its lanes passes alone -- the plan is the narrow
   * build's (16 utterances per wavefront, the one-wave kernel whatever the tuning asks for, no group table), its ring takes
   * every wavefront's longest cycle, ring and cos rows of the worst wavefront fit the LDS and are what lds_one_wave says,
   * every wavefront of 16 has one threshold, every launch picks the narrow build; and a refusal is never the policy's whim:
   * the smallest ring and the worst wavefront's cos rows do not fit */
  {
    const size_t sizes[] = {1, 15, 16, 17, 33, 4200, 20000};
    const vs_tuning tunes[] = {{0}, {.ring_slots = 24}, {.ring_slots = 600}, {.kernel = VS_KERNEL_WS}};
    vs_lane *src = (vs_lane *)malloc(n * sizeof(vs_lane));
    VsDevLane *rec = (VsDevLane *)malloc(n * sizeof(VsDevLane));
    CHECK(src != NULL && rec != NULL);
    long accepted = 0, refused = 0, shallow = 0, many_rows = 0;
    for (int kind = 0; kind < LB_KINDS; kind++)
      for (size_t si = 0; si < (kind < LB_REFUSED ? sizeof(sizes) / sizeof(sizes[0]) : kind == LB_REFUSED ? 1 : N_REFUSED); si++) {
        const size_t m = kind < LB_REFUSED ? sizes[si] : kind == LB_REFUSED ? N_REFUSED : 1;
        long_batch(kind, src, m, si);
        VsBatchStats st;
        VsPlanTables tab;
        CHECK(vs_expand_all_ordered(src, rec, m, NULL, &st) == VS_OK);
        CHECK(vs_plan_tables_build(src, rec, m, &st, 0, &tab) == VS_OK);
        int ring = 0, worst_rows = 0;
        const size_t need = narrow_need(rec, m, &ring, &worst_rows);
        /* (every batch of this loop has a lane beyond the 64-column ring, but the 44.1 kHz lanes of the refused batch alone) */
        const int narrow = st.tmax > 1152 - VS_SS - VS_TRASH_ROWS;
        CHECK(narrow || kind == LB_REFUSED_ALONE);
        CHECK(tab.ltab_entries >= worst_rows || !narrow);
        if (worst_rows >= 12 * 160 && m >= 16) many_rows++; /* (a dozen rows and more in some wavefront) */
        for (size_t ti = 0; ti < sizeof(tunes) / sizeof(tunes[0]); ti++)
          for (int cus = 8; cus <= 256; cus += 248) {
            const vs_tuning *t = &tunes[ti];
            VsPlanShape sh;
            dealt_calls = 0;
            const int rc = vs_plan_shape(rec, m, 4000, &st, 0, cus, t, tab.ltab_entries, dealt_stub, NULL, &sh);
            CHECK(rc == VS_OK || rc == VS_ERR_UNSUPPORTED);
            CHECK((rc == VS_ERR_UNSUPPORTED) == (kind == LB_REFUSED));
            if (rc == VS_ERR_UNSUPPORTED) {
              refused++;
              CHECK(need > VS_LDS_LIMIT || ring > (int)((VS_LDS_LIMIT - 16 * 1024) / (VS_NARROW_LANES * 2) / VS_SS) * VS_SS);
            }
            if (rc == VS_OK && narrow) {
              accepted++;
              CHECK(need <= VS_LDS_LIMIT);
              CHECK(sh.group_lanes == VS_NARROW_LANES && sh.grid == (m + 15) / 16);
              CHECK(!sh.wave_specialised && sh.gmap == NULL && sh.n_wg_mixed == 0 && dealt_calls == 0);
              CHECK(sh.ring_slots % VS_SS == 0 && sh.ring_slots >= ring && sh.ltab_entries == tab.ltab_entries);
              CHECK(sh.lds_one_wave == (size_t)(sh.ring_slots + VS_TRASH_ROWS) * 32 + (size_t)sh.ltab_entries * 8);
              CHECK(sh.lds_one_wave <= VS_LDS_LIMIT && sh.lds_bytes == sh.lds_one_wave);
              if (t->ring_slots == 24) CHECK(sh.ring_slots == ring); /* the least a plan can be asked for: the smallest ring */
              for (size_t w0 = 0; w0 < m; w0 += VS_NARROW_LANES) {
                int tb = 1, sum = 0, seen_t2[VS_NARROW_LANES], ns = 0;
                for (size_t l = w0; l < m && l < w0 + VS_NARROW_LANES; l++) {
                  if (rec[l].tbound > tb) tb = rec[l].tbound;
                  CHECK(rec[l].ready_min == rec[w0].ready_min); /* one threshold per wavefront of 16 */
                  int dup = 0;
                  for (int q = 0; q < ns; q++) dup |= seen_t2[q] == rec[l].T2;
                  if (!dup) {
                    seen_t2[ns++] = rec[l].T2;
                    sum += (rec[l].T2 + 7) & ~7;
                  }
                }
                const int thr = rec[w0].ready_min;
                CHECK(thr == 32 || thr == 48 || thr == 58 || thr == 64);
                CHECK(sh.ring_slots >= VS_SS + tb + VS_TRASH_ROWS && sh.ltab_entries >= sum);
                const double rho = (double)(sh.ring_slots - VS_SS) / (double)tb;
                CHECK(thr == (rho >= 1.65 ? 64 : rho >= 1.45 ? 58 : rho >= 1.33 ? 48 : 32));
                if (thr < 64) shallow++;
              }
              for (int arith = VS_ARITH_EXACT; arith <= VS_ARITH_F32; arith++)
                for (int lk = VS_KIND_SYNTH; lk <= VS_KIND_FILTER; lk++)
                  for (int log = 0; log <= (lk != VS_KIND_FILTER); log++) {
                    VsKernelArgs a;
                    memset(&a, 0, sizeof(a));
                    a.group_lanes = sh.group_lanes;
                    a.ws_roles = sh.ws_roles;
                    a.ws_pairs = sh.ws_pairs;
                    VsLaunchPick p = {0, 0, 0, 0};
                    CHECK(vs_launch_pick(arith, lk, log != 0, sh.wave_specialised != 0, sh.pre1 != 0, &a, sh.grid, sh.lds_one_wave, &p) == 0);
                    const int one = arith == VS_ARITH_EXACT ? VS_ARITH_EXACT : VS_ARITH_FMA;
                    CHECK(VS_KERNEL_FAMILY(p.kernel) == VS_KF_NARROW && p.block == VS_WAVE && p.grid == sh.grid);
                    CHECK(p.lds_bytes == (lk == VS_KIND_FILTER ? 0 : sh.lds_one_wave));
                    CHECK(p.kernel == VS_KERNEL_ID(VS_KF_NARROW, lk == VS_KIND_SOURCE ? VS_ARITH_EXACT : one, lk, log,
                                                   lk != VS_KIND_SOURCE && one == VS_ARITH_EXACT && sh.pre1));
                  }
            }
            free(sh.gmap);
          }
        vs_plan_tables_release(&tab);
      }
    /* the loop saw what it is for: plans and refusals, wavefronts under every kind of threshold, wavefronts with a dozen
     * cos rows and more */
    CHECK(accepted >= 3 * 7 * 8 && refused == 8 && shallow > 1000 && many_rows >= 5);
    free(src);
    free(rec);
  }

  /* which kernel a launch runs, with what block, grid and LDS: the selection against the copy of the launchers it
   * replaced, over everything they could be given -- and a little more (arithmetic 3, kind 3: no such kernel) */
  {
    static const int roles[] = {0, 2, 3}, pairs[] = {0, 1, 2, 4}, glanes[] = {0, 64, 16};
    static const size_t ldss[] = {0, 48 * 1024, 48 * 1024 + 8, 160 * 1024};
    static const unsigned grids[] = {1, 3, 4, 5, 65535, 0x7FFFFFFFu};
    float some_ondw = 0;
    int32_t some_odone = 0;
    VsGroupSlot some_map = {0, 0, 0, 0};
    long cases = 0, refused = 0, div0 = 0;
    for (int arith = 0; arith <= 3; arith++)
    for (int kind = 0; kind <= 3; kind++)
    for (int sel = 0; sel < 8; sel++) /* log, wave_specialised, pre1 */
    for (int ri = 0; ri < 3; ri++)
    for (int pi = 0; pi < 4; pi++)
    for (int layout = VS_WS_LAYOUT_ROLE_MAJOR; layout <= VS_WS_LAYOUT_SPREAD_2X3; layout++)
    for (int map = 0; map <= 1; map++)
    for (int gi = 0; gi < 3; gi++)
    for (int on = 0; on < 8; on++) /* ondw, odone, pow_lframe > 0 */
    for (int li = 0; li < 4; li++)
    for (int di = 0; di < 6; di++) {
      const bool log = sel & 1, ws = (sel & 2) != 0, pre1 = (sel & 4) != 0;
      VsKernelArgs a;
      memset(&a, 0, sizeof(a));
      a.group_lanes = glanes[gi];
      a.ws_roles = roles[ri];
      a.ws_pairs = pairs[pi];
      a.ws_layout = layout;
      a.ws_pair_bytes = 38208 + 16 * li;
      a.group_map = map ? &some_map : NULL;
      a.ondw = (on & 1) ? &some_ondw : NULL;
      a.odone = (on & 2) ? &some_odone : NULL;
      a.pow_lframe = (on & 4) ? 800 : 0;
      const Was w = was_launch(false, arith, kind, log, ws, pre1, &a, grids[di], ldss[li]);
      VsLaunchPick p = {0, 0, 0, 0};
      const int rc = vs_launch_pick(arith, kind, log, ws, pre1, &a, grids[di], ldss[li], &p);
      cases++;
      refused += w.refused;
      div0 += w.div0;
      if (w.refused || w.div0) {
        CHECK(rc != 0);
      } else {
        CHECK(rc == 0 && p.kernel == w.fn && p.block == w.block && p.grid == w.grid && p.lds_bytes == w.lds_bytes);
      }
      if (ri + pi + layout + map + on == 0) { /* the narrow launcher, which reads none of those */
        const Was wn = was_launch(true, arith, kind, log, false, pre1, &a, grids[di], ldss[li]);
        const int rn = vs_launch_pick_narrow(arith, kind, log, pre1, grids[di], ldss[li], &p);
        CHECK((rn != 0) == wn.refused);
        if (rn == 0) CHECK(p.kernel == wn.fn && p.block == wn.block && p.grid == wn.grid && p.lds_bytes == wn.lds_bytes);
      }
      if (fails > 20) goto picks_done; /* (a wrong rule is wrong in thousands of places) */
    }
  picks_done:
    CHECK(cases == 4L * 4 * 8 * 3 * 4 * 2 * 2 * 3 * 8 * 4 * 6 && refused > 0 && div0 > 0);
    /* the wide filter: exact, or the fused multiply-adds for both other arithmetics; not without its taps and an input */
    for (int arith = 0; arith <= 2; arith++)
      for (int have = 0; have < 4; have++) {
        VsKernelArgs a;
        double taps = 0;
        int16_t in = 0;
        memset(&a, 0, sizeof(a));
        a.awide = (have & 1) ? &taps : NULL;
        a.in = (have & 2) ? &in : NULL;
        VsLaunchPick p = {0, 0, 0, 0};
        CHECK((vs_launch_pick_wide(arith, &a, 7, &p) == 0) == (have == 3));
        CHECK(p.kernel == VS_KERNEL_ID(VS_KF_WIDE, arith == VS_ARITH_EXACT ? VS_ARITH_EXACT : VS_ARITH_FMA, 0, 0, 0) && p.block == VS_WAVE && p.grid == 7 && p.lds_bytes == 0);
      }
    char name[64];
    vs_kernel_id_name(VS_KERNEL_ID(VS_KF_WS_POW, 2, 1, 3, 0), name, sizeof(name));
    CHECK(!strcmp(name, "vs_synth_ws_pow_kernel<2, true, 3>"));
    vs_kernel_id_name(VS_KERNEL_ID(VS_KF_NARROW, 0, 1, 1, 0), name, sizeof(name));
    CHECK(!strcmp(name, "vs_synth_kernel<0, 1, true, false>"));

    /* vowel -n's two passes: rows of 1 .. 4096 blocks and of the most a row can have (2^31 - 1 samples), and as many
     * rows as make nblocks = segs * n_lanes the smallest it can be (one row), twice that, the largest value below 2^31,
     * and the first value beyond it (refused); both power passes, both store widths */
    for (long segs = 1; segs <= 4097; segs++) {
      const long s = segs <= 4096 ? segs : ((0x7FFFFFFFL + 2047) / 2048);
      const long lanes_max = 0x7FFFFFC0L; /* the most a plan takes (vs_plan_create): the fill pass rounds them up to 64 in an int */
      const long most = 0x7FFFFFFFL / s < lanes_max ? 0x7FFFFFFFL / s : lanes_max;
      const long rows[] = {1, 2, most, most + 1};
      for (int r = 0; r < 4; r++) {
        if (rows[r] > lanes_max) continue;
        VsKernelArgs a;
        memset(&a, 0, sizeof(a));
        a.ondw = &some_ondw;
        a.ondw_pitch = 1 + (segs % 3);
        a.odone = (segs & 1) ? &some_odone : NULL;
        a.vec_ok = (segs & 2) ? 1 : 0;
        a.n_lanes = (int)rows[r];
        a.n_samples = (int)(s * 2048 > 0x7FFFFFFFL ? 0x7FFFFFFFL : s * 2048 - (segs % 5));
        check_out_noise(&a, 1, 1);
        if (r < 2 && segs <= 4096) {
          check_out_noise(&a, 1, 0); /* the measurement builds: a two-dimensional grid, two octets per thread */
          check_out_noise(&a, 2, 1);
        }
      }
    }
    {
      VsKernelArgs a;
      memset(&a, 0, sizeof(a));
      a.n_lanes = 1 << 20;
      a.n_samples = 16000;
      a.ondw_pitch = 1 << 20; /* 2^40 frames: more power blocks than a grid holds */
      check_out_noise(&a, 1, 1); /* no table */
      a.ondw = &some_ondw;
      check_out_noise(&a, 1, 1);
      a.ondw_pitch = 0;
      check_out_noise(&a, 1, 1);
      a.ondw_pitch = 20;
      a.n_samples = 65536 * 2048; /* 65536 segments: one too many for the second dimension of a grid */
      a.n_lanes = 3;
      check_out_noise(&a, 1, 0);
      check_out_noise(&a, 1, 1);
    }
  }

  /* two bad lanes met by different threads: the lowest one's error is the answer */
  lanes[17000].F0 = 10.0f;                   /* below 50: VS_ERR_RANGE */
  lanes[3000].cq = 0.0f;                     /* no pulse: VS_ERR_UNSUPPORTED */
  CHECK(vs_expand_all(lanes, dl, n, 0) == VS_ERR_UNSUPPORTED);
  CHECK(vs_expand_all_ordered(lanes, dl, n, NULL, NULL) == VS_ERR_UNSUPPORTED); /* ... in kernel order too: lane 3000 is the lowest */
  lanes[3000].cq = 0.55f;
  CHECK(vs_expand_all(lanes, dl, n, 0) == VS_ERR_RANGE);
  CHECK(vs_expand_all_ordered(lanes, dl, n, NULL, NULL) == VS_ERR_RANGE);
  lanes[17000].F0 = 120.0f;
  CHECK(vs_expand_all(lanes, dl, n, 1) == VS_OK);  /* the filter-only records */

  /* ring policy: every period, both ring widths, caps and explicit requests */
  for (int tmax = 1; tmax <= 5200; tmax += (tmax < 300 ? 1 : 37)) {
    int slots = 0, thr = 0;
    for (int cap = 0; cap <= 1200; cap += 300) {
      for (int req = 0; req <= 1; req++) {
        const int rc = vs_ring_policy_for(VS_WAVE, tmax, cap, &slots, &thr, req ? cap : 0, req ? 2.4 : 1.7);
        if (rc == VS_OK) CHECK(slots % VS_SS == 0 && slots >= VS_SS + tmax + VS_TRASH_ROWS && (size_t)(slots + VS_TRASH_ROWS) * 128 <= VS_LDS_LIMIT);
        else CHECK(rc == VS_ERR_UNSUPPORTED);
      }
    }
    const int rc = vs_ring_slots_for(tmax, &slots);
    CHECK(rc == VS_OK || rc == VS_ERR_UNSUPPORTED);
  }
  double row[257];
  vs_cos_row(257, row);
  CHECK(row[0] == 1.0 && row[256] < -0.99);

  /* the rounds of a node's gather */
  for (int shards = 1; shards <= 9; shards++) {
    const size_t total = 100003, chunk = 4096;
    size_t covered = 0;
    const size_t rounds = vs_gather_rounds(total, shards, chunk);
    for (int s = 0; s < shards; s++) {
      size_t lo, hi, nxt;
      CHECK(vs_shard_cut(total, shards, s, &lo, &hi) == VS_OK);
      nxt = lo;
      for (size_t k = 0; k < rounds + 2; k++) {
        size_t r0, rows;
        CHECK(vs_gather_round(total, shards, s, chunk, k, &r0, &rows) == VS_OK);
        if (rows) {
          CHECK(r0 == nxt && rows <= chunk);
          nxt += rows;
        }
      }
      CHECK(nxt == hi);
      covered += hi - lo;
    }
    CHECK(covered == total);
  }
  free(lanes);
  free(dl);
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
