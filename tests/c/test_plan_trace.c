/* What synthesis plans send across the library's two lower boundaries -- the HIP runtime and the kernel launchers -- written
 * out as text: vs_api.c, vs_blocks.c, vs_planhost.c and vs_host.c as they are, against the stand-in runtime of
 * hip_standin.h and stand-in launchers that print what they are given.  Per case: the return codes, the public getters,
 * every device / pinned allocation with its size, every copy (direction, bytes, where to, a hash of the bytes, which
 * stream), the probe launches, and for every launch the launcher, its selectors, grid, LDS bytes, stream and every field
 * of VsKernelArgs (the first launch of a case in full, the later ones as the fields that differ from it).  Pointers are
 * NULL or "a<allocation serial>+<offset>".  The hashes of the record block and of the small block carry ready_min,
 * tab_off, tap_row, the cos rows, the taps and the group table.
 * With --full the program prints all of that.  Without, a digest: per case its name, the lines that say what kind of plan
 * came out (create, info, what is live after destroy) and the number of lines and a 64-bit hash of the case's full text.
 * tests/golden/plan_trace.txt is the digest; tests/test_host_sanitizers.py builds the program under ASan/UBSan and
 * compares byte for byte.  When a case differs: --full of both trees, and diff.  Host logic only.
 * The stand-in launchers also ask the selection of vs_planhost.c which kernels the real ones would launch for what they were
 * given; the case behind "end" holds, for every launch without a log of the cases above it, vs_plan_kernel_name next to that
 * answer.  The recording is only ever appended to: the long-period cases (the narrow build) follow, with a list of their own. */
#define STANDIN_COPY_DOWN 1
#define STANDIN_FILL 0xA5
#include "../../voice_synth_amd/csrc/vs_internal.h"
#include "hip_standin.h"

/* a case writes its text into memory; end_case prints it, or its digest */
static FILE *trace;
static char *trace_text;
static size_t trace_len;
static int full_text;
static void begin_case(void)
{
  trace = open_memstream(&trace_text, &trace_len);
  if (!trace) exit(2);
}
static void end_case(int whole)
{
  fclose(trace);
  if (full_text || whole) {
    fwrite(trace_text, 1, trace_len, stdout);
  } else {
    int lines = 0, first = 1;
    for (const char *l = trace_text; *l; l = strchr(l, '\n') + 1, lines++, first = 0)
      if (first || !strncmp(l, "  create:", 9) || !strncmp(l, "  info:", 7) || !strncmp(l, "  live after", 12) || !strncmp(l, "  names:", 8))
        fwrite(l, 1, (size_t)(strchr(l, '\n') + 1 - l), stdout);
    fprintf(stdout, "  trace: %d lines, hash %016llx\n", lines, standin_hash(trace_text, trace_len));
  }
  free(trace_text);
}
#define printf(...) fprintf(trace, __VA_ARGS__)

static vs_ctx *cur; /* the context of the case: names the streams */
static char launch_stream, pipeline_stream;

static const char *ptr_str(const void *p, char *buf)
{
  size_t off = 0;
  const int k = p ? standin_find(p, &off) : -1;
  if (!p) snprintf(buf, 48, "NULL");
  else if (k < 0) snprintf(buf, 48, "host");
  else snprintf(buf, 48, "a%d+%zu", k, off);
  return buf;
}
static const char *stream_str(hipStream_t s)
{
  if (!s) return "null";
  if (cur && s == cur->stream) return "launch";
  if (cur && s == cur->own_upload) return "own";
  if (cur && s == cur->upload) return "pipeline";
  return "other";
}

/* ---- the launchers: print, launch nothing ---- */
#define MAX_FIELDS 48
typedef struct Field {
  const char *name;
  char val[64];
} Field;
static Field first_launch[MAX_FIELDS];
static int have_first;
static int quiet;        /* the injection rounds: launchers say nothing */
static int hash_records; /* zero-copy plans: nothing is copied, so the launch hashes the block its records lie in */
static int last_vec_ok;  /* what the last launcher was given (alignments() reads it under quiet) */

/* the kernels the selection names for the launches since picked[0] = 0, " + " between them */
static char picked[256];
static void note_kernel(int rc, int id)
{
  const size_t used = strlen(picked);
  char one[64];
  vs_kernel_id_name(id, one, sizeof(one));
  snprintf(picked + used, sizeof(picked) - used, "%s%s%s", used ? " + " : "", rc ? "REFUSED " : "", one);
}

static void print_launch(const char *launcher, int arith, int kind, int log, int ws, int pre1, const VsKernelArgs *a,
                         unsigned grid, size_t lds, hipStream_t s)
{
  Field f[MAX_FIELDS];
  int n = 0;
  char b[48];
  last_vec_ok = a->vec_ok;
  if (quiet) return;
#define F_INT(nm, v) (f[n].name = nm, snprintf(f[n].val, sizeof(f[n].val), "%ld", (long)(v)), n++)
#define F_PTR(nm, v) (f[n].name = nm, snprintf(f[n].val, sizeof(f[n].val), "%s", ptr_str(v, b)), n++)
#define F_STR(nm, v) (f[n].name = nm, snprintf(f[n].val, sizeof(f[n].val), "%s", v), n++)
  F_STR("launcher", launcher);
  F_INT("arith", arith);
  F_INT("kind", kind);
  F_INT("log", log);
  F_INT("ws", ws);
  F_INT("pre1", pre1);
  F_INT("grid", grid);
  F_INT("lds", lds);
  F_STR("stream", stream_str(s));
  F_PTR("a.lanes", a->lanes);
  F_PTR("a.costab", a->costab);
  F_PTR("a.in", a->in);
  F_PTR("a.out", a->out);
  F_PTR("a.log", a->log);
  F_PTR("a.ncyc", a->ncyc);
  F_INT("a.in_pitch", a->in_pitch);
  F_INT("a.out_pitch", a->out_pitch);
  F_INT("a.log_pitch", a->log_pitch);
  F_INT("a.n_lanes", a->n_lanes);
  F_INT("a.n_samples", a->n_samples);
  F_INT("a.ring_slots", a->ring_slots);
  F_INT("a.vec_ok", a->vec_ok);
  F_INT("a.ltab_entries", a->ltab_entries);
  F_INT("a.ready_min", a->ready_min);
  F_INT("a.ws_pairs", a->ws_pairs);
  F_INT("a.ws_roles", a->ws_roles);
  F_INT("a.group_lanes", a->group_lanes);
  F_INT("a.ws_pair_bytes", a->ws_pair_bytes);
  F_INT("a.gen_min", a->gen_min);
  F_PTR("a.ondw", a->ondw);
  F_INT("a.ondw_pitch", a->ondw_pitch);
  F_PTR("a.odone", a->odone);
  F_INT("a.pow_lframe", a->pow_lframe);
  F_INT("a.gen_low", a->gen_low);
  F_PTR("a.err", a->err);
  F_INT("a.spin_limit", a->spin_limit);
  F_INT("a.fault", a->fault);
  F_INT("a.ws_filter_prio", a->ws_filter_prio);
  F_PTR("a.diag", a->diag);
  F_PTR("a.sink", a->sink);
  F_PTR("a.awide", a->awide);
  F_INT("a.ws_layout", a->ws_layout);
  F_PTR("a.taps", a->taps);
  F_PTR("a.group_map", a->group_map);
  printf(have_first ? "    ->" : "    -> (in full)");
  for (int k = 0; k < n; k++)
    if (!have_first || strcmp(f[k].val, first_launch[k].val) != 0) printf(" %s=%s", f[k].name, f[k].val);
  printf("\n");
  if (!have_first) memcpy(first_launch, f, sizeof(f));
  have_first = 1;
  if (hash_records) {
    size_t off = 0;
    const int k = standin_find(a->lanes, &off);
    if (k >= 0) printf("       block a%d holds %016llx\n", k, standin_hash(alloc_log[k].ptr, alloc_log[k].bytes));
  }
}

hipError_t vs_launch_kernel(int arith, int kind, bool log, bool wave_specialised, bool pre1, const VsKernelArgs *args,
                            unsigned grid, size_t lds_bytes, hipStream_t stream)
{
  VsLaunchPick pick = {0, 0, 0, 0};
  const int refused = vs_launch_pick(arith, kind, log, wave_specialised, pre1, args, grid, lds_bytes, &pick);
  note_kernel(refused, pick.kernel);
  print_launch("kernel", arith, kind, log, wave_specialised, pre1, args, grid, lds_bytes, stream);
  return hipSuccess;
}
hipError_t vs_launch_filter_wide(int arith, const VsKernelArgs *args, unsigned grid, hipStream_t stream)
{
  VsLaunchPick pick = {0, 0, 0, 0};
  const int refused = vs_launch_pick_wide(arith, args, grid, &pick);
  note_kernel(refused, pick.kernel);
  print_launch("filter_wide", arith, -1, -1, -1, -1, args, grid, 0, stream);
  return hipSuccess;
}
hipError_t vs_launch_out_noise(const VsKernelArgs *args, hipStream_t stream)
{
  VsOutNoisePick pick;
  memset(&pick, 0, sizeof(pick));
  const int rc = vs_launch_pick_out_noise(args, 1, 1, &pick);
  note_kernel(rc, pick.power.kernel);
  note_kernel(rc, pick.noise.kernel);
  print_launch("out_noise", -1, -1, -1, -1, -1, args, 0, 0, stream);
  return hipSuccess;
}
hipError_t vs_launch_reseed(VsDevLane *lanes, const unsigned long long *seeds, const unsigned long long *out_seeds,
                            int n_lanes, hipStream_t stream)
{
  return hipSuccess;
}
hipError_t vs_launch_selftest(unsigned long long *bad_dev, hipStream_t stream) { return hipSuccess; }

/* the probe: HW_ID words that are dealt four at a time (wavefront w on SIMD w % 4 of CU g), or all on SIMD 0, or a launch
 * that fails */
enum { PROBE_DEALT, PROBE_NOT_DEALT, PROBE_FAILS };
static int probe_answer, probe_launches;
hipError_t vs_launch_simd_probe(int waves, unsigned grid, size_t lds_bytes, unsigned *out_dev, hipStream_t stream)
{
  probe_launches++;
  if (!quiet) printf("  probe launch: %d wavefronts, grid %u, lds %zu, stream %s\n", waves, grid, lds_bytes, stream_str(stream));
  if (probe_answer == PROBE_FAILS) return hipErrorLaunchFailure;
  for (unsigned g = 0; g < grid; g++)
    for (int w = 0; w < waves; w++)
      out_dev[(size_t)g * 16 + (size_t)w] =
          0x80000000u | ((g & 0xFFu) << 8) | ((probe_answer == PROBE_DEALT ? (unsigned)(w & 3) : 0u) << 4);
  return hipSuccess;
}

/* of csrc/vs_delivery.c, which is not part of this program: the one pool buffer a plan can grow */
void vs_pool_release(vs_ctx *ctx)
{
  if (ctx->pool.d_flow) (void)hipFree(ctx->pool.d_flow);
  ctx->pool.d_flow = NULL;
  ctx->pool.d_flow_bytes = 0;
}

/* ---- the batches ---- */
enum { B_CONFIG1, B_CONFIG2, B_CONFIG3, B_CONFIG4, B_SWEEP, B_NARROW, B_192K, B_WIDE, B_NARROW_HET, B_REFUSED };
#define B_ONOISE 0x100      /* every lane asks for vowel -n */
#define B_WIDE_SETS 0x800   /* every third lane carries a coefficient set of 40 taps */
#define B_TWO_FRAMES 0x200  /* ... and every third lane runs at 22050 Hz: two frame lengths */
#define B_LOW_FS 0x400      /* ... and lane 5 runs below 2000 Hz, without -n: no frame at all */
static vs_lane *make_lanes(int batch, size_t n)
{
  vs_lane *lanes = (vs_lane *)malloc(n * sizeof(vs_lane));
  if (!lanes) exit(2);
  for (size_t i = 0; i < n; i++) {
    vs_lane *l = &lanes[i];
    vs_lane_defaults(l);
    l->fs = 16000;
    l->seed = 1 + i;
    const int kind = batch & 0xFF;
    if (kind != B_CONFIG1) {
      l->flags |= VS_FLAG_JITTER | VS_FLAG_SHIMMER;
      l->jitter = 0.01f;
      l->shimmer = 0.1f;
    }
    if (kind != B_CONFIG1 && kind != B_CONFIG2) {
      l->flags |= VS_FLAG_NOISE;
      l->noise = 100.0f;
      l->vowel = "12467"[i % 5];
    }
    if (kind == B_CONFIG4) l->fs = 22050;
    if (kind == B_SWEEP) {
      l->F0 = 80.0f + 220.0f * (float)((i * 2654435761u) & 0xFFFF) / 65536.0f;
      l->Fg = l->F0 * 125.0f / 120.0f + 1.0f;
    }
    if (kind == B_NARROW || kind == B_192K) {
      l->fs = kind == B_NARROW ? 48000 : 192000;
      l->F0 = 50.0f;
      l->Fg = 52.0f;
    }
    if (kind == B_NARROW_HET) {
      /* long periods, every lane with source options of its own (tests/c/test_planhost_asan.c, long_lane): 48 .. 64 kHz,
       * F0 50 .. 55 Hz, cq 0.30 .. 0.89, jitter, shimmer and glottal noise on and off */
      static const int rates[4] = {64000, 56000, 48000, 50000};
      l->fs = rates[i % 4];
      l->F0 = 50.0f + 5.0f * (float)((7 * i) % 1013) / 1012.0f;
      l->Fg = l->F0 * 125.0f / 120.0f + 1.0f;
      l->cq = 0.30f + 0.59f * (float)((13 * i) % 1021) / 1020.0f;
      l->flags = 0;
      if (i % 4 != 3) l->flags |= VS_FLAG_JITTER;
      l->jitter = 0.03f;
      if (i % 3) l->flags |= VS_FLAG_SHIMMER;
      if (i & 1) l->flags |= VS_FLAG_NOISE;
      if (i % 7 == 2) l->pre_emphasis = 0.5f;
    }
    if (kind == B_REFUSED) {
      /* the 15 lanes of tests/c/test_planhost_asan.c, refused_spec: each passes alone, together they are refused */
      static const struct { int fs; float F0, Fg, cq; } spec[15] = {
          {176400, 50.0f, 52.0f, 0.30f}, {176400, 56.0f, 58.0f, 0.35f}, {176400, 64.0f, 66.0f, 0.42f}, {176400, 79.0f, 81.0f, 0.45f},
          {96000, 50.0f, 52.0f, 0.55f},  {96000, 52.0f, 54.0f, 0.60f},  {96000, 55.0f, 57.0f, 0.65f},  {96000, 60.0f, 62.0f, 0.70f},
          {88200, 50.0f, 52.0f, 0.75f},  {88200, 53.0f, 55.0f, 0.80f},  {88200, 58.0f, 60.0f, 0.85f},  {88200, 66.0f, 68.0f, 0.89f},
          {44100, 50.0f, 52.0f, 0.85f},  {44100, 51.0f, 53.0f, 0.89f},  {44100, 79.0f, 81.0f, 0.80f}};
      vs_lane_defaults(l);
      l->fs = spec[i % 15].fs;
      l->F0 = spec[i % 15].F0;
      l->Fg = spec[i % 15].Fg;
      l->cq = spec[i % 15].cq;
      l->seed = 900 + i;
    }
    if (kind == B_WIDE || ((batch & B_WIDE_SETS) && i % 3 == 0)) {
      l->vowel = VS_VOWEL_CUSTOM;
      l->order = 40;
      for (int j = 1; j <= 40; j++) l->A[j] = ((j & 1) ? -0.5 : 0.25) / (double)(j + (int)(i % 3));
    }
    if (batch & B_ONOISE) {
      l->out_snr = 100.0f;
      l->out_seed = 77 + i;
    }
    if ((batch & B_TWO_FRAMES) && i % 3 == 2) l->fs = 22050;
    if ((batch & B_LOW_FS) && i == 5) {
      l->fs = 1900;
      l->F0 = 50.0f;
      l->Fg = 52.0f;
      l->out_snr = 0.0f;
    }
  }
  return lanes;
}

/* ---- one case ---- */
typedef struct Case {
  const char *name;
  int batch;
  size_t n_lanes, n_samples;
  int mode;        /* VS_PLAN_* */
  int cus;         /* 0: 256 */
  int probe;       /* PROBE_* */
  int pipeline;    /* the context has a pipeline's upload stream */
  vs_tuning tune;
  int filter_rows; /* ... and launches of the filter-only kind on rows of their own pitches, in every arithmetic */
} Case;

static vs_ctx *open_ctx(const Case *c)
{
  vs_ctx *ctx = NULL;
  standin_cu_count = c->cus ? c->cus : 256;
  probe_answer = c->probe;
  if (vs_ctx_create(0, &ctx) != VS_OK) exit(2);
  vs_ctx_set_stream(ctx, &launch_stream);
  if (c->pipeline) ctx->upload = (hipStream_t)&pipeline_stream;
  const int rc = vs_ctx_set_tuning(ctx, &c->tune);
  if (rc != VS_OK) printf("  set_tuning: %d\n", rc);
  cur = ctx;
  return ctx;
}

/* the last case's text, gathered while the others run */
static FILE *names;
static int names_launches, names_differ;

static void launch(vs_plan *p, int kind, int arith, int with_log, size_t out_pitch, void *bufs[4], size_t n_samples)
{
  vs_ctx_set_arith(cur, arith);
  char name[256] = "";
  vs_plan_kernel_name(p, kind, name, sizeof(name));
  picked[0] = 0;
  printf("  launch kind %d arith %d log %d out_pitch %zu: %s\n", kind, arith, with_log, out_pitch, name);
  const int rc = vs_plan_launch(p, kind, kind == VS_KIND_FILTER ? (const int16_t *)bufs[0] : NULL, n_samples + 8,
                                (int16_t *)bufs[1], out_pitch, with_log ? (vs_cycle_rec *)bufs[2] : NULL, with_log ? 400 : 0,
                                with_log ? (int32_t *)bufs[3] : NULL);
  printf("    rc %d\n", rc);
  if (!with_log && rc == VS_OK) { /* (the name is that of the launch without a log) */
    /* the name carries a remark behind the narrow build's kernel, which is no part of the kernel's name */
    char bare[256];
    snprintf(bare, sizeof(bare), "%s", name);
    char *remark = strstr(bare, " (narrow build: 16 utterances per wavefront)");
    if (remark) memmove(remark, remark + 44, strlen(remark + 44) + 1);
    const int same = !strcmp(bare, picked);
    names_launches++;
    names_differ += !same;
    fprintf(names, "    kind %d arith %d out_pitch %zu: %s | %s%s\n", kind, arith, out_pitch, name, picked, same ? "" : " | DIFFER");
  }
}

static void print_traffic(void)
{
  char b[48];
  for (int k = 0; k < n_allocs && k < STANDIN_ALLOC_LOG; k++)
    printf("  alloc a%d: %s %zu bytes\n", k, alloc_log[k].kind == 'd' ? "device" : "pinned", alloc_log[k].bytes);
  for (int k = 0; k < n_copies && k < STANDIN_COPY_LOG; k++) {
    const StandinCopy *c = &copy_log[k];
    if (c->alloc < 0) snprintf(b, sizeof(b), "host");
    else snprintf(b, sizeof(b), "a%d+%zu", c->alloc, c->off);
    printf("  copy %d: %c %zu bytes, device side %s, hash %016llx, stream %s\n", k, c->kind, c->bytes, b, c->hash, stream_str(c->stream));
  }
  if (n_allocs > STANDIN_ALLOC_LOG || n_copies > STANDIN_COPY_LOG) printf("  LOG FULL\n");
}

static void reset_logs(void)
{
  calls = fail_at = n_allocs = n_copies = probe_launches = have_first = 0;
  failed_fn = NULL;
}

static void run_case(const Case *c)
{
  reset_logs();
  printf("== %s\n", c->name);
  fprintf(names, "  %s\n", c->name);
  /* the caller's device arrays first, so that they are a0..a3 in every case: in, out, cycle log, cycle counts */
  void *bufs[4];
  for (int k = 0; k < 4; k++)
    if (hipMalloc(&bufs[k], 64) != hipSuccess) exit(2);
  vs_lane *lanes = make_lanes(c->batch, c->n_lanes);
  vs_ctx *ctx = open_ctx(c);
  vs_plan *p = NULL;
  const int rc = vs_plan_create_impl(ctx, lanes, c->n_lanes, c->n_samples, c->mode, &p);
  printf("  create: %d, hip error %d\n", rc, vs_ctx_last_hip_error(ctx));
  if (rc == VS_OK) {
    size_t lds = 0, wgs = 0, slots = 0;
    int roles = 0, layout = 0, fallback = 0;
    vs_plan_info(p, &lds, &wgs, &slots);
    vs_plan_roles(p, &roles, &layout, &fallback);
    printf("  info: lds %zu, workgroups %zu, ring slots %zu; roles %d, layout %d, simd fallback %d\n", lds, wgs, slots, roles,
           layout, fallback);
    hash_records = (c->mode & VS_PLAN_ZERO_COPY) != 0;
    const size_t pitch = (c->n_samples + 7) & ~(size_t)7;
    for (int arith = VS_ARITH_EXACT; arith <= VS_ARITH_F32; arith++) {
      for (int kind = VS_KIND_SYNTH; kind <= VS_KIND_FILTER; kind++)
        for (int with_log = 0; with_log <= (kind != VS_KIND_FILTER); with_log++) launch(p, kind, arith, with_log, pitch, bufs, c->n_samples);
    }
    launch(p, (c->mode & VS_PLAN_FILTER_ONLY) ? VS_KIND_FILTER : VS_KIND_SYNTH, VS_ARITH_EXACT, 0, c->n_samples | 1, bufs, c->n_samples);
    if (c->filter_rows)
      for (int arith = VS_ARITH_EXACT; arith <= VS_ARITH_F32; arith++) launch(p, VS_KIND_FILTER, arith, 0, c->n_samples + 2 + (size_t)arith, bufs, c->n_samples);
    hash_records = 0;
    int flags = -1;
    const int src = vs_plan_status(p, &flags);
    printf("  status: %d, flags %d\n", src, flags);
  }
  printf("  probe launches: %d\n", probe_launches);
  print_traffic();
  vs_plan_destroy(p);
  vs_ctx_destroy(ctx);
  cur = NULL;
  for (int k = 0; k < 4; k++) (void)hipFree(bufs[k]);
  printf("  live after destroy: device %d, pinned %d, events %d, streams %d\n", dev_live, pin_live, ev_live, stream_live);
  free(lanes);
}

/* every runtime call of one create - launch - destroy round fails in turn */
static void run_injection(const Case *c)
{
  printf("== failure injection: %s\n", c->name);
  vs_lane *lanes = make_lanes(c->batch, c->n_lanes);
  void *out = NULL;
  int n_calls = 0;
  for (int k = 0; k <= n_calls; k++) { /* k = 0: the clean round that counts the calls */
    reset_logs();
    if (hipMalloc(&out, 64) != hipSuccess) exit(2);
    vs_ctx *ctx = open_ctx(c);
    vs_plan *p = NULL;
    calls = 0;
    fail_at = k;
    const int crc = vs_plan_create_impl(ctx, lanes, c->n_lanes, c->n_samples, c->mode, &p);
    int lrc = -99;
    quiet = 1; /* (what the launches are given is in the cases' own traces) */
    if (crc == VS_OK) lrc = vs_plan_launch(p, VS_KIND_SYNTH, NULL, 0, (int16_t *)out, c->n_samples, NULL, 0, NULL);
    vs_plan_destroy(p);
    quiet = 0;
    if (k == 0) n_calls = calls;
    fail_at = 0;
    const int herr = vs_ctx_last_hip_error(ctx);
    vs_ctx_destroy(ctx);
    cur = NULL;
    (void)hipFree(out);
    printf("  fail_at %d (%s): create %d, launch %d, hip error %d, %d allocations, %d copies; live device %d, pinned %d, events %d, streams %d\n",
           k, failed_fn ? failed_fn : "-", crc, lrc, herr, n_allocs, n_copies, dev_live, pin_live, ev_live, stream_live);
  }
  free(lanes);
}

static void refusals(void)
{
  printf("== argument refusals\n");
  reset_logs();
  const Case c = {"refusals", B_CONFIG2, 70, 16000, 0, 0, 0, 0, {0}};
  vs_lane *lanes = make_lanes(c.batch, c.n_lanes);
  vs_ctx *ctx = open_ctx(&c);
  vs_plan *p = NULL, *pf = NULL;
  void *in = NULL, *out = NULL;
  if (hipMalloc(&in, 64) != hipSuccess || hipMalloc(&out, 64) != hipSuccess) exit(2);
  printf("  create, no context: %d\n", vs_plan_create_impl(NULL, lanes, 70, 16000, 0, &p));
  printf("  create, no lanes: %d\n", vs_plan_create_impl(ctx, NULL, 70, 16000, 0, &p));
  printf("  create, no plan pointer: %d\n", vs_plan_create_impl(ctx, lanes, 70, 16000, 0, NULL));
  printf("  create, 0 lanes: %d\n", vs_plan_create_impl(ctx, lanes, 0, 16000, 0, &p));
  printf("  create, 0 samples: %d\n", vs_plan_create_impl(ctx, lanes, 70, 0, 0, &p));
  printf("  create, too many lanes: %d\n", vs_plan_create_impl(ctx, lanes, (size_t)0x7FFFFFC1, 16000, 0, &p));
  printf("  create, too many samples: %d\n", vs_plan_create_impl(ctx, lanes, 70, (size_t)0x7FFFFF01, 0, &p));
  printf("  runtime calls so far: %d\n", calls);
  lanes[33].F0 = 10.0f;
  printf("  create, F0 out of range: %d, plan %s\n", vs_plan_create_impl(ctx, lanes, 70, 16000, 0, &p), p ? "set" : "NULL");
  lanes[33].F0 = 120.0f;
  lanes[12].cq = 0.0f;
  printf("  create, no pulse: %d\n", vs_plan_create_impl(ctx, lanes, 70, 16000, 0, &p));
  lanes[12].cq = 0.55f;
  printf("  create: %d\n", vs_plan_create_impl(ctx, lanes, 70, 16000, 0, &p));
  printf("  create, filter only: %d\n", vs_plan_create_impl(ctx, lanes, 70, 16000, VS_PLAN_FILTER_ONLY, &pf));
  const int before = calls;
  int16_t *i16 = (int16_t *)in, *o16 = (int16_t *)out;
  printf("  launch, no plan: %d\n", vs_plan_launch(NULL, VS_KIND_SYNTH, NULL, 0, o16, 16000, NULL, 0, NULL));
  printf("  launch, no output: %d\n", vs_plan_launch(p, VS_KIND_SYNTH, NULL, 0, NULL, 16000, NULL, 0, NULL));
  printf("  launch, kind 7: %d\n", vs_plan_launch(p, 7, NULL, 0, o16, 16000, NULL, 0, NULL));
  printf("  launch, short out_pitch: %d\n", vs_plan_launch(p, VS_KIND_SYNTH, NULL, 0, o16, 15999, NULL, 0, NULL));
  printf("  launch, filter without input: %d\n", vs_plan_launch(p, VS_KIND_FILTER, NULL, 16000, o16, 16000, NULL, 0, NULL));
  printf("  launch, filter with short in_pitch: %d\n", vs_plan_launch(p, VS_KIND_FILTER, i16, 15999, o16, 16000, NULL, 0, NULL));
  printf("  launch, filter-only plan as synth: %d\n", vs_plan_launch(pf, VS_KIND_SYNTH, NULL, 0, o16, 16000, NULL, 0, NULL));
  printf("  launch, log without pitch: %d\n", vs_plan_launch(p, VS_KIND_SYNTH, NULL, 0, o16, 16000, (vs_cycle_rec *)in, 0, NULL));
  printf("  runtime calls of the refused launches: %d\n", calls - before);
  vs_plan_destroy(p);
  vs_plan_destroy(pf);
  vs_ctx_destroy(ctx);
  cur = NULL;
  (void)hipFree(in);
  (void)hipFree(out);
  printf("  live after destroy: device %d, pinned %d, events %d, streams %d\n", dev_live, pin_live, ev_live, stream_live);
  free(lanes);
}

/* 16-byte loads and stores are allowed when every row of BOTH arrays starts 4-byte aligned: the base and the pitch of the
 * output, and for the filter-only kind of the input as well */
static void alignments(void)
{
  printf("== row alignment: vec_ok by kind, in base + bytes / in_pitch, out base + bytes / out_pitch\n");
  reset_logs();
  const Case cs[2] = {{"fused", B_CONFIG2, 70, 1000, 0, 0, 0, 0, {0}}, {"wide", B_WIDE, 70, 1000, 0, 0, 0, 0, {0}}};
  void *in = NULL, *out = NULL;
  if (hipMalloc(&in, 64) != hipSuccess || hipMalloc(&out, 64) != hipSuccess) exit(2);
  if ((((uintptr_t)in) | ((uintptr_t)out)) & 15) exit(2);
  static const struct { int kind, in_off; size_t in_pitch; int out_off; size_t out_pitch; } L[] = {
      {VS_KIND_FILTER, 0, 1008, 0, 1008}, {VS_KIND_FILTER, 0, 1002, 0, 1008}, {VS_KIND_FILTER, 0, 1008, 0, 1002},
      {VS_KIND_FILTER, 0, 1001, 0, 1000}, {VS_KIND_FILTER, 0, 1000, 0, 1001}, {VS_KIND_FILTER, 2, 1008, 0, 1008},
      {VS_KIND_FILTER, 0, 1008, 2, 1008}, {VS_KIND_FILTER, 2, 1002, 2, 1002}, {VS_KIND_FILTER, 4, 1002, 4, 1002},
      {VS_KIND_SYNTH, 2, 1001, 0, 1002},  {VS_KIND_SYNTH, 0, 1008, 2, 1008},  {VS_KIND_SYNTH, 0, 1008, 0, 1003}};
  for (int c = 0; c < 2; c++) {
    vs_lane *lanes = make_lanes(cs[c].batch, cs[c].n_lanes);
    vs_ctx *ctx = open_ctx(&cs[c]);
    vs_plan *p = NULL;
    printf("  %s plan: create %d\n", cs[c].name, vs_plan_create_impl(ctx, lanes, cs[c].n_lanes, cs[c].n_samples, 0, &p));
    quiet = 1;
    for (size_t k = 0; p && k < sizeof(L) / sizeof(L[0]); k++) {
      last_vec_ok = -1;
      const int rc = vs_plan_launch(p, L[k].kind, (const int16_t *)((char *)in + L[k].in_off), L[k].in_pitch,
                                    (int16_t *)((char *)out + L[k].out_off), L[k].out_pitch, NULL, 0, NULL);
      printf("    kind %d, in +%d / %zu, out +%d / %zu: rc %d, vec_ok %d\n", L[k].kind, L[k].in_off, L[k].in_pitch, L[k].out_off,
             L[k].out_pitch, rc, last_vec_ok);
    }
    quiet = 0;
    vs_plan_destroy(p);
    vs_ctx_destroy(ctx);
    cur = NULL;
    free(lanes);
  }
  (void)hipFree(in);
  (void)hipFree(out);
  printf("  live after destroy: device %d, pinned %d, events %d, streams %d\n", dev_live, pin_live, ev_live, stream_live);
}

#define T0 {0}
int main(int argc, char **argv)
{
  full_text = argc > 1 && !strcmp(argv[1], "--full");
  const size_t sweep_n = 65536 - 219;
  char *names_text = NULL;
  size_t names_len = 0;
  names = open_memstream(&names_text, &names_len);
  if (!names) return 2;
  const Case cases[] = {
      /* name, batch, lanes, samples, mode, CUs, probe, pipeline, tuning */
      {"config 1: one lane", B_CONFIG1, 1, 16000, 0, 0, 0, 0, T0},
      {"config 2: 1024 lanes", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, T0},
      {"config 2 on a pipeline's upload stream", B_CONFIG2, 1024, 16000, 0, 0, 0, 1, T0},
      {"config 3: 65536 lanes (full grid, role-major)", B_CONFIG3, 65536, 16000, 0, 0, 0, 0, T0},
      {"config 4's shard: 32768 lanes at 22050 Hz, 2 s (spread layout)", B_CONFIG4, 32768, 44100, 0, 0, 0, 0, T0},
      {"config 3, 16384 lanes (a SIMD per wavefront)", B_CONFIG3, 16384, 16000, 0, 0, 0, 0, T0},
      {"F0 sweep, 65317 lanes (mixed rings, ragged last group)", B_SWEEP, sweep_n, 16000, 0, 0, 0, 0, T0},
      {"F0 sweep, mixed_rings -1", B_SWEEP, sweep_n, 16000, 0, 0, 0, 0, {.mixed_rings = -1}},
      {"F0 sweep, mixed_rings 200", B_SWEEP, sweep_n, 16000, 0, 0, 0, 0, {.mixed_rings = 200}},
      {"F0 sweep, mixed_rings 600 (does not fit)", B_SWEEP, sweep_n, 16000, 0, 0, 0, 0, {.mixed_rings = 600}},
      {"8 CUs, 1100 lanes of config 3", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, T0},
      {"8 CUs, 1100 lanes of the F0 sweep", B_SWEEP, 1100, 16000, 0, 8, 0, 0, T0},
      {"8 CUs, 2100 lanes of config 3 (four groups per workgroup)", B_CONFIG3, 2100, 16000, 0, 8, 0, 0, T0},
      {"8 CUs, 2100 lanes of the F0 sweep", B_SWEEP, 2100, 16000, 0, 8, 0, 0, T0},
      {"8 CUs, 2100 lanes of the F0 sweep, uniform rings", B_SWEEP, 2100, 16000, 0, 8, 0, 0, {.mixed_rings = -1}},
      {"8 CUs, 2100 lanes of config 3, kernel SINGLE", B_CONFIG3, 2100, 16000, 0, 8, 0, 0, {.kernel = VS_KERNEL_SINGLE}},
      {"8 CUs, 2100 lanes of config 3, roles 2", B_CONFIG3, 2100, 16000, 0, 8, 0, 0, {.ws_roles = 2}},
      {"8 CUs, 500 lanes of config 3 (half grid)", B_CONFIG3, 500, 16000, 0, 8, 0, 0, T0},
      {"8 CUs, 300 lanes of the F0 sweep (one group per workgroup)", B_SWEEP, 300, 16000, 0, 8, 0, 0, T0},
      /* the probe's other answers */
      {"full grid, not dealt four at a time", B_CONFIG3, 65536, 16000, 0, 0, PROBE_NOT_DEALT, 0, T0},
      {"full grid, VS_FAULT_SIMD_DEALING", B_CONFIG3, 65536, 16000, 0, 0, 0, 0, {.fault = VS_FAULT_SIMD_DEALING}},
      {"full grid, the probe fails", B_CONFIG3, 65536, 16000, 0, 0, PROBE_FAILS, 0, T0},
      {"half grid, not dealt four at a time", B_CONFIG4, 32768, 44100, 0, 0, PROBE_NOT_DEALT, 0, T0},
      {"half grid, VS_FAULT_SIMD_DEALING", B_CONFIG4, 32768, 44100, 0, 0, 0, 0, {.fault = VS_FAULT_SIMD_DEALING}},
      {"half grid, the probe fails", B_CONFIG4, 32768, 44100, 0, 0, PROBE_FAILS, 0, T0},
      {"mixed rings on 8 CUs, not dealt four at a time", B_SWEEP, 1100, 16000, 0, 8, PROBE_NOT_DEALT, 0, T0},
      /* tuning: on a full grid of 8 CUs, on a half grid, on config 2 */
      {"tuning kernel SINGLE, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.kernel = VS_KERNEL_SINGLE}},
      {"tuning kernel SINGLE, config 2", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, {.kernel = VS_KERNEL_SINGLE}},
      {"tuning kernel WS roles 2, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.kernel = VS_KERNEL_WS, .ws_roles = 2}},
      {"tuning kernel WS roles 3, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.kernel = VS_KERNEL_WS, .ws_roles = 3}},
      {"tuning kernel WS roles 2, half grid", B_CONFIG3, 500, 16000, 0, 8, 0, 0, {.kernel = VS_KERNEL_WS, .ws_roles = 2}},
      {"tuning kernel WS roles 3, F0 sweep with uniform rings", B_SWEEP, 1100, 16000, 0, 8, 0, 0, {.kernel = VS_KERNEL_WS, .ws_roles = 3, .mixed_rings = -1}},
      {"tuning kernel WS roles 2, mixed rings", B_SWEEP, 1100, 16000, 0, 8, 0, 0, {.kernel = VS_KERNEL_WS, .ws_roles = 2}},
      {"tuning ws_pairs 1, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.ws_pairs = 1}},
      {"tuning ws_pairs 2, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.ws_pairs = 2}},
      {"tuning ws_pairs 4, config 2", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, {.ws_pairs = 4}},
      {"tuning ws_pairs 2, F0 sweep", B_SWEEP, 1100, 16000, 0, 8, 0, 0, {.ws_pairs = 2}},
      {"tuning ws_pairs 4, F0 sweep", B_SWEEP, 1100, 16000, 0, 8, 0, 0, {.ws_pairs = 4}},
      {"tuning ring_slots 240, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.ring_slots = 240}},
      {"tuning ring_slots 600, F0 sweep", B_SWEEP, 1100, 16000, 0, 8, 0, 0, {.ring_slots = 600}},
      {"tuning ring_slots 4000, config 2", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, {.ring_slots = 4000}},
      {"tuning ready_min 50, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.ready_min = 50}},
      {"tuning ready_min 50, config 2", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, {.ready_min = 50}},
      {"tuning gen_min 20 gen_low 100, full grid", B_CONFIG3, 1100, 16000, 0, 8, 0, 0, {.gen_min = 20, .gen_low = 100}},
      {"tuning gen_min 20 gen_low 100, half grid", B_CONFIG3, 500, 16000, 0, 8, 0, 0, {.gen_min = 20, .gen_low = 100}},
      {"tuning gen_min 20, mixed rings", B_SWEEP, 1100, 16000, 0, 8, 0, 0, {.gen_min = 20}},
      {"tuning gen_low 100, mixed rings", B_SWEEP, 1100, 16000, 0, 8, 0, 0, {.gen_low = 100}},
      {"tuning ws_filter_prio -1", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, {.ws_filter_prio = -1}},
      {"tuning ws_filter_prio 2", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, {.ws_filter_prio = 2}},
      {"tuning spin_limit 1000", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, {.spin_limit = 1000}},
      /* the other kinds of plan */
      {"filter-only plan", B_CONFIG3, 1024, 16000, VS_PLAN_FILTER_ONLY, 0, 0, 0, T0},
      {"wide plan (order 40)", B_WIDE, 200, 16000, 0, 0, 0, 0, T0},
      {"wide plan, filter only", B_WIDE, 200, 16000, VS_PLAN_FILTER_ONLY, 0, 0, 0, T0},
      {"wide plan with VS_PLAN_POOL_SCRATCH", B_WIDE, 200, 16000, VS_PLAN_POOL_SCRATCH, 0, 0, 0, T0},
      {"zero-copy plan", B_CONFIG3, 5, 16000, VS_PLAN_ZERO_COPY, 0, 0, 0, T0},
      {"zero-copy wide plan", B_WIDE, 3, 16000, VS_PLAN_ZERO_COPY, 0, 0, 0, T0},
      {"zero-copy F0 sweep with mixed rings", B_SWEEP, 1100, 16000, VS_PLAN_ZERO_COPY, 8, 0, 0, T0},
      {"narrow build: 48 kHz, F0 50 / Fg 52", B_NARROW, 100, 48000, 0, 0, 0, 0, T0},
      {"a period beyond the narrow build: 192 kHz", B_192K, 4, 192000, 0, 0, 0, 0, T0},
      {"vowel -n, one frame length (the pow kernel)", B_CONFIG3 | B_ONOISE, 1024, 16000, 0, 0, 0, 0, T0},
      {"vowel -n, one frame length, full grid", B_CONFIG3 | B_ONOISE, 1100, 16000, 0, 8, 0, 0, T0},
      {"vowel -n, two frame lengths", B_CONFIG3 | B_ONOISE | B_TWO_FRAMES, 1024, 16000, 0, 0, 0, 0, T0},
      {"vowel -n, a lane below 2000 Hz", B_CONFIG3 | B_ONOISE | B_LOW_FS, 1024, 16000, 0, 0, 0, 0, T0},
      {"vowel -n, filter only with a lane below 2000 Hz", B_CONFIG3 | B_ONOISE | B_LOW_FS, 1024, 16000, VS_PLAN_FILTER_ONLY, 0, 0, 0, T0},
      {"vowel -n, kernel SINGLE", B_CONFIG3 | B_ONOISE, 1024, 16000, 0, 0, 0, 0, {.kernel = VS_KERNEL_SINGLE}},
  };
  for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); k++) {
    begin_case();
    run_case(&cases[k]);
    end_case(0);
  }
  begin_case();
  refusals();
  end_case(1);
  const Case inject[] = {
      {"config 2: 1024 lanes", B_CONFIG2, 1024, 16000, 0, 0, 0, 0, T0},
      {"F0 sweep, 65317 lanes (mixed rings)", B_SWEEP, sweep_n, 16000, 0, 0, 0, 0, T0},
      {"wide plan (order 40)", B_WIDE, 200, 16000, 0, 0, 0, 0, T0},
      {"wide plan with VS_PLAN_POOL_SCRATCH", B_WIDE, 200, 16000, VS_PLAN_POOL_SCRATCH, 0, 0, 0, T0},
      {"zero-copy F0 sweep with mixed rings", B_SWEEP, 1100, 16000, VS_PLAN_ZERO_COPY, 8, 0, 0, T0},
  };
  for (size_t k = 0; k < sizeof(inject) / sizeof(inject[0]); k++) {
    begin_case();
    run_injection(&inject[k]);
    end_case(0);
  }
  begin_case();
  alignments();
  end_case(1);
  fprintf(stdout, "end\n");
  /* (behind the recording's last line: the recording is only ever appended to) */
  fclose(names);
  begin_case();
  printf("== kernel names: vs_plan_kernel_name | the kernels the selection gave the launchers of that launch\n");
  printf("%s", names_text);
  printf("  names: %d launches, %d differ\n", names_launches, names_differ);
  end_case(0);
  free(names_text);
  /* ---- appended to the recording: long periods (the narrow build) ---- */
  const int first_differ = names_differ;
  names_launches = names_differ = 0;
  names = open_memstream(&names_text, &names_len);
  if (!names) return 2;
  const Case narrow[] = {
      {"narrow build, 33 lanes of their own periods (two whole wavefronts of 16 and one lane)", B_NARROW_HET, 33, 4000, 0, 0, 0, 0, T0},
      {"narrow build, 33 lanes, ring_slots 24 (the smallest ring)", B_NARROW_HET, 33, 4000, 0, 0, 0, 0, {.ring_slots = 24}},
      {"narrow build, 33 lanes with vowel -n", B_NARROW_HET | B_ONOISE, 33, 5000, 0, 0, 0, 0, T0},
      {"narrow build, 33 lanes with wide sets (the wide filter behind the narrow source kernel)", B_NARROW_HET | B_WIDE_SETS, 33, 4000, 0, 0, 0, 0, T0},
      {"narrow build, 17 lanes, filter kind on rows of its own pitches", B_NARROW_HET, 17, 4000, 0, 0, 0, 0, T0, 1},
      {"narrow build, 4200 lanes on 8 CUs (shallow rings)", B_NARROW_HET, 4200, 3000, 0, 8, 0, 0, T0},
      {"15 lanes that pass alone and are refused together", B_REFUSED, 15, 6000, 0, 0, 0, 0, T0},
      {"... the first of them alone", B_REFUSED, 1, 6000, 0, 0, 0, 0, T0},
  };
  for (size_t k = 0; k < sizeof(narrow) / sizeof(narrow[0]); k++) {
    begin_case();
    run_case(&narrow[k]);
    end_case(0);
  }
  fclose(names);
  begin_case();
  printf("== kernel names of the long-period cases\n");
  printf("%s", names_text);
  printf("  names: %d launches, %d differ\n", names_launches, names_differ);
  end_case(0);
  free(names_text);
  return (first_differ || names_differ) ? 1 : 0;
}
