/* The host-buffer calls (vs_host_begin / vs_host_end and vs_pool_device of csrc/vs_blocks.c, and the five calls built on
 * them: vs_measure, vs_lpc, vs_iaif, vs_track, vs_inverse) against the stand-in HIP runtime of hip_standin.h.  The
 * kernels' launchers are stand-ins too: they note the device arrays they are given and launch nothing.
 * Checked: for each of the five calls, with every optional array and with none, that the copies and fills on the
 * context's stream are the ones include/voice_synth.h documents (written out below from its array shapes), that the
 * arrays the launch sees lie apart, 256-byte aligned, inside what d_aux was grown for, and that an absent array reaches
 * the launch as NULL; for every runtime call of a begin / end round -- on a fresh pool and on one that must grow -- that
 * failing it gives VS_ERR_HIP, leaves the context usable and leaks nothing; that d_aux is asked for the parts' rounded
 * sizes to the byte; a launch that refuses.
 * Host logic only, under ASan/UBSan with leak detection (tests/test_host_sanitizers.py). */
#define STANDIN_COPY_DOWN 1
#include "../../voice_synth_amd/csrc/vs_blocks.c"
#include "../../voice_synth_amd/csrc/vs_acoustic.h"
#include "../../voice_synth_amd/csrc/vs_iaif.h"
#include "../../voice_synth_amd/csrc/vs_inverse.h"
#include "hip_standin.h"

/* ---- the stand-in launchers: [0] the input, then the call's arrays in the order of its signature ---- */
#define MAX_ARGS 5
static const void *seen[MAX_ARGS];
static int launches;
static void see(const void *a0, const void *a1, const void *a2, const void *a3, const void *a4)
{
  const void *a[MAX_ARGS] = {a0, a1, a2, a3, a4};
  memcpy(seen, a, sizeof(seen));
  launches++;
}
hipError_t vs_launch_measure(const VsAcArgs *a, int lds_doubles, hipStream_t s)
{
  see(a->pcm, a->out, a->marks, NULL, NULL);
  return hipSuccess;
}
hipError_t vs_launch_lpc(const VsLpcArgs *a, hipStream_t s)
{
  see(a->pcm, a->frames, a->formants, a->coefs, NULL);
  return hipSuccess;
}
hipError_t vs_launch_iaif(const VsIaifArgs *a, hipStream_t s)
{
  see(a->lpc.pcm, a->lpc.frames, a->lpc.formants, a->lpc.coefs, a->glottal);
  return hipSuccess;
}
hipError_t vs_launch_track(int arith, int mode, const VsTrackArgs *a, hipStream_t s)
{
  see(a->in, a->out, a->coefs, a->gains, a->stat);
  return hipSuccess;
}
hipError_t vs_launch_inverse(int arith, int mode, const VsInverseArgs *a, hipStream_t s)
{
  see(a->in, a->out, a->coefs, a->stat, NULL);
  return hipSuccess;
}

static char the_stream;

static vs_ctx *new_ctx(void)
{
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(vs_ctx));
  if (!ctx) exit(2);
  ctx->stream = (hipStream_t)&the_stream;
  calls = fail_at = n_copies = launches = stream_syncs = 0;
  return ctx;
}

static void release(vs_ctx *ctx)
{
  VsRecSlot *slots[5] = {&ctx->rec_measure, &ctx->rec_lpc, &ctx->rec_track, &ctx->rec_inverse, &ctx->rec_iaif};
  for (int k = 0; k < 5; k++) vs_rec_release(ctx, slots[k]);
  vs_plan_cache_release(ctx);
  if (ctx->own_upload) (void)hipStreamDestroy(ctx->own_upload);
  (void)hipFree(ctx->pool.d_in);
  (void)hipFree(ctx->pool.d_aux);
  CHECK(dev_live == 0 && pin_live == 0 && ev_live == 0 && stream_live == 0);
  free(ctx);
}

static size_t room(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

/* ---- the five calls: what moves, and where the launch's arrays lie ---- */

typedef struct Want {
  char kind; /* 'U' up, 'D' down, 'F' fill */
  size_t bytes;
  int arg;   /* the array it moves: index into seen[] */
} Want;

/* After one successful call on a fresh context.  arg_bytes[k]: the documented size of seen[k], 0 = the call was made
 * without it.  want: the traffic on the context's stream, in order. */
static void check_call(vs_ctx *ctx, int rc, const Want *want, int n_want, const size_t *arg_bytes, int n_args)
{
  CHECK(rc == VS_OK && launches == 1 && stream_syncs == 1 && ctx->last_hip_error == 0);
  const char *d_in = (const char *)ctx->pool.d_in, *aux = (const char *)ctx->pool.d_aux;
  /* the launch's arrays: the input at the start of d_in; the others apart, aligned, inside what d_aux was asked for */
  size_t asked = 0;
  for (int k = 1; k < n_args; k++) asked += arg_bytes[k] ? room(arg_bytes[k]) : 0;
  CHECK(seen[0] == d_in && ctx->pool.d_in_bytes == (size_t)1 << 20 && arg_bytes[0] <= ctx->pool.d_in_bytes);
  CHECK(ctx->pool.d_aux_bytes == (size_t)1 << 20 && asked <= ctx->pool.d_aux_bytes);
  for (int k = 1; k < MAX_ARGS; k++) {
    if (k >= n_args || arg_bytes[k] == 0) {
      CHECK(seen[k] == NULL);
      continue;
    }
    const size_t off = (size_t)((const char *)seen[k] - aux);
    CHECK(seen[k] != NULL && (const char *)seen[k] >= aux && off % 256 == 0 && off + arg_bytes[k] <= asked);
    for (int j = 1; j < k; j++) {
      if (!arg_bytes[j]) continue;
      const size_t offj = (size_t)((const char *)seen[j] - aux);
      CHECK(off >= offj + arg_bytes[j] || offj >= off + arg_bytes[k]);
    }
  }
  /* the traffic: the record upload of the launch on a stream of its own, everything else on the context's, as wanted */
  CHECK(n_copies <= STANDIN_COPY_LOG);
  int n = 0, elsewhere = 0;
  for (int c = 0; c < n_copies; c++) {
    const StandinCopy *got = &copy_log[c];
    if (got->stream != ctx->stream) {
      CHECK(got->kind == 'U' && got->stream == ctx->own_upload);
      elsewhere++;
      continue;
    }
    CHECK(n < n_want);
    if (got->kind != want[n].kind || got->bytes != want[n].bytes || got->dev != seen[want[n].arg]) {
      printf("copy %d: %c %zu bytes at %s+%zu, wanted %c %zu of array %d\n", n, got->kind, got->bytes,
             want[n].arg ? "d_aux" : "d_in", (size_t)((const char *)got->dev - (want[n].arg ? aux : d_in)), want[n].kind,
             want[n].bytes, want[n].arg);
      exit(1);
    }
    n++;
  }
  CHECK(n == n_want && elsewhere == 1);
  release(ctx);
}
#define N(a) ((int)(sizeof(a) / sizeof((a)[0])))

static void measure_calls(void)
{
  /* 3 rows of 64 samples at a pitch of 70; vs_acoustic: 96 bytes; marks [3][8] int32 */
  enum { ROWS = 3, PITCH = 70, NS = 64, MP = 8 };
  int16_t *pcm = (int16_t *)calloc((ROWS - 1) * PITCH + NS, sizeof(int16_t));
  vs_acoustic *out = (vs_acoustic *)calloc(ROWS, 96);
  int32_t *marks = (int32_t *)calloc(ROWS * MP, sizeof(int32_t));
  const int32_t fs[ROWS] = {16000, 16000, 8000};
  CHECK(pcm && out && marks && sizeof(vs_acoustic) == 96);

  vs_ctx *ctx = new_ctx();
  const Want all[] = {{'U', 408, 0}, {'F', 96, 2}, {'D', 288, 1}, {'D', 96, 2}};
  const size_t all_bytes[] = {408, 288, 96};
  check_call(ctx, vs_measure(ctx, NULL, pcm, PITCH, ROWS, NS, fs, NULL, out, marks, MP), all, N(all), all_bytes, 3);
  CHECK(marks[0] == -1 && marks[ROWS * MP - 1] == -1); /* the fill came back */

  ctx = new_ctx();
  const Want none[] = {{'U', 408, 0}, {'D', 288, 1}};
  const size_t none_bytes[] = {408, 288, 0};
  check_call(ctx, vs_measure(ctx, NULL, pcm, PITCH, ROWS, NS, fs, NULL, out, NULL, 0), none, N(none), none_bytes, 3);

  /* a launch that refuses (a rate outside the lag limits) after begin: waited for, its code returned, nothing comes down */
  ctx = new_ctx();
  const int32_t bad_fs[ROWS] = {16000, 10, 16000};
  CHECK(vs_measure(ctx, NULL, pcm, PITCH, ROWS, NS, bad_fs, NULL, out, marks, MP) == VS_ERR_RANGE);
  CHECK(launches == 0 && stream_syncs == 1 && n_copies == 2 && copy_log[0].kind == 'U' && copy_log[1].kind == 'F');
  release(ctx);
  free(pcm);
  free(out);
  free(marks);
}

static void frame_calls(void)
{
  /* 2 rows of 800 samples at a pitch of 810 and 16 kHz: 3 frames of 400 samples every 160, frames_pitch 4.
   * vs_lpc_frame: 32 bytes; formants [2][4][2 * 5], coefs [2][4][22 + 1], glottal [2][4][4 + 1] doubles */
  enum { ROWS = 2, PITCH = 810, NS = 800, FP = 4 };
  int16_t *pcm = (int16_t *)calloc((ROWS - 1) * PITCH + NS, sizeof(int16_t));
  vs_lpc_frame *frames = (vs_lpc_frame *)calloc(ROWS * FP, 32);
  double *formants = (double *)calloc(ROWS * FP * 2 * 5, sizeof(double));
  double *coefs = (double *)calloc(ROWS * FP * 23, sizeof(double));
  double *glottal = (double *)calloc(ROWS * FP * 5, sizeof(double));
  const int32_t fs[ROWS] = {16000, 16000};
  CHECK(pcm && frames && formants && coefs && glottal && sizeof(vs_lpc_frame) == 32);

  vs_ctx *ctx = new_ctx();
  const Want all[] = {{'U', 3220, 0}, {'U', 256, 1}, {'U', 640, 2}, {'U', 1472, 3}, {'D', 256, 1}, {'D', 640, 2}, {'D', 1472, 3}};
  const size_t all_bytes[] = {3220, 256, 640, 1472};
  check_call(ctx, vs_lpc(ctx, NULL, pcm, PITCH, ROWS, NS, fs, NULL, FP, frames, formants, coefs), all, N(all), all_bytes, 4);

  ctx = new_ctx();
  const Want none[] = {{'U', 3220, 0}, {'U', 256, 1}, {'D', 256, 1}};
  const size_t none_bytes[] = {3220, 256, 0, 0};
  check_call(ctx, vs_lpc(ctx, NULL, pcm, PITCH, ROWS, NS, fs, NULL, FP, frames, NULL, NULL), none, N(none), none_bytes, 4);

  /* n_formants == 0: a formants array that is given is absent all the same */
  ctx = new_ctx();
  vs_lpc_opts o;
  CHECK(vs_lpc_defaults(&o) == VS_OK);
  o.n_formants = 0;
  const Want nof[] = {{'U', 3220, 0}, {'U', 256, 1}, {'U', 1472, 3}, {'D', 256, 1}, {'D', 1472, 3}};
  const size_t nof_bytes[] = {3220, 256, 0, 1472};
  check_call(ctx, vs_lpc(ctx, &o, pcm, PITCH, ROWS, NS, fs, NULL, FP, frames, formants, coefs), nof, N(nof), nof_bytes, 4);

  ctx = new_ctx();
  const Want iall[] = {{'U', 3220, 0}, {'U', 256, 1}, {'U', 640, 2}, {'U', 1472, 3}, {'U', 320, 4},
                       {'D', 256, 1},  {'D', 640, 2}, {'D', 1472, 3}, {'D', 320, 4}};
  const size_t iall_bytes[] = {3220, 256, 640, 1472, 320};
  check_call(ctx, vs_iaif(ctx, NULL, pcm, PITCH, ROWS, NS, fs, NULL, FP, frames, formants, coefs, glottal), iall, N(iall),
             iall_bytes, 5);

  ctx = new_ctx();
  const size_t inone_bytes[] = {3220, 256, 0, 0, 0};
  check_call(ctx, vs_iaif(ctx, NULL, pcm, PITCH, ROWS, NS, fs, NULL, FP, frames, NULL, NULL, NULL), none, N(none),
             inone_bytes, 5);
  free(pcm);
  free(frames);
  free(formants);
  free(coefs);
  free(glottal);
}

static void setwalk_calls(void)
{
  /* 3 rows of 100 samples, 2 sets of order 4 per row: coefs [3][2][4 + 1] and gains [3][2] doubles; vs_track_stat: 8
   * bytes, vs_inverse_stat: 16 */
  enum { ROWS = 3, NS = 100, SP = 2, ORDER = 4 };
  int16_t *in = (int16_t *)calloc(ROWS * NS, sizeof(int16_t)), *out = (int16_t *)calloc(ROWS * NS, sizeof(int16_t));
  double *coefs = (double *)calloc(ROWS * SP * (ORDER + 1), sizeof(double));
  double *gains = (double *)calloc(ROWS * SP, sizeof(double));
  vs_track_stat tstat[ROWS];
  vs_inverse_stat istat[ROWS];
  vs_track_row trows[ROWS];
  vs_inverse_row irows[ROWS];
  CHECK(in && out && coefs && gains && sizeof(tstat) == 24 && sizeof(istat) == 48);
  for (int i = 0; i < ROWS; i++) {
    trows[i] = (vs_track_row){SP, 50, 0, NS - i, 1.0f, 0.0f};
    irows[i] = (vs_inverse_row){SP, 50, 0, NS - i, 1.0f, 0.0f};
  }

  vs_ctx *ctx = new_ctx();
  const Want all[] = {{'U', 600, 0}, {'U', 600, 1}, {'U', 240, 2}, {'U', 48, 3}, {'D', 600, 1}, {'D', 24, 4}};
  const size_t all_bytes[] = {600, 600, 240, 48, 24};
  check_call(ctx, vs_track(ctx, VS_TRACK_HOLD, ORDER, in, out, ROWS, NS, trows, coefs, gains, SP, tstat), all, N(all),
             all_bytes, 5);

  ctx = new_ctx();
  const Want none[] = {{'U', 600, 0}, {'U', 600, 1}, {'U', 240, 2}, {'D', 600, 1}};
  const size_t none_bytes[] = {600, 600, 240, 0, 0};
  check_call(ctx, vs_track(ctx, VS_TRACK_GLIDE, ORDER, in, out, ROWS, NS, trows, coefs, NULL, SP, NULL), none, N(none),
             none_bytes, 5);

  ctx = new_ctx();
  const Want iall[] = {{'U', 600, 0}, {'U', 600, 1}, {'U', 240, 2}, {'D', 600, 1}, {'D', 48, 3}};
  const size_t iall_bytes[] = {600, 600, 240, 48};
  check_call(ctx, vs_inverse(ctx, VS_TRACK_HOLD, ORDER, in, out, ROWS, NS, irows, coefs, SP, istat), iall, N(iall),
             iall_bytes, 4);

  ctx = new_ctx();
  const size_t inone_bytes[] = {600, 600, 240, 0};
  check_call(ctx, vs_inverse(ctx, VS_TRACK_GLIDE, ORDER, in, out, ROWS, NS, irows, coefs, SP, NULL), none, N(none),
             inone_bytes, 4);

  /* the checks stay in front of every runtime call, the rows' own last */
  ctx = new_ctx();
  irows[1].de_emphasis = 1.5f;
  CHECK(vs_inverse(ctx, VS_TRACK_HOLD, ORDER, in, out, ROWS, NS, irows, coefs, SP, NULL) == VS_ERR_RANGE);
  trows[2].n_sets = SP + 1;
  CHECK(vs_track(ctx, VS_TRACK_HOLD, ORDER, in, out, ROWS, NS, trows, coefs, NULL, SP, NULL) == VS_ERR_RANGE);
  CHECK(vs_track(ctx, 7, ORDER, in, out, ROWS, NS, trows, coefs, NULL, SP, NULL) == VS_ERR_ARG);
  CHECK(vs_track(ctx, VS_TRACK_HOLD, ORDER, in, out, ROWS, NS, trows, coefs, NULL, (size_t)1 << 31, NULL) == VS_ERR_UNSUPPORTED);
  CHECK(calls == 0);
  release(ctx);
  free(in);
  free(out);
  free(coefs);
  free(gains);
}

/* ---- the helper itself: every runtime call of a round fails in turn; a launch that refuses ---- */

/* a round on a table of every kind of part; scale sizes it.  The DOWN parts must come back as the "device" holds them:
 * what went up, or the fill */
static int one_round(vs_ctx *ctx, size_t scale, int launch_rc)
{
  const size_t in_bytes = 1000 * scale, a_bytes = 300 * scale, b_bytes = 77 * scale, c_bytes = 500 * scale;
  char *in = (char *)malloc(in_bytes), *a = (char *)malloc(a_bytes), *b = (char *)malloc(b_bytes),
       *c = (char *)malloc(c_bytes), absent;
  if (!in || !a || !b || !c) exit(2);
  memset(in, 1, in_bytes);
  memset(a, 2, a_bytes);
  memset(b, 3, b_bytes);
  memset(c, 4, c_bytes);
  VsHostPart parts[5] = {{a, a_bytes, VS_PART_UP | VS_PART_DOWN, NULL},
                         {NULL, 64, VS_PART_UP | VS_PART_DOWN, NULL},
                         {b, b_bytes, VS_PART_FILL_FF | VS_PART_DOWN, NULL},
                         {&absent, 0, VS_PART_UP, NULL},
                         {c, c_bytes, VS_PART_UP, NULL}};
  int rc = vs_host_begin(ctx, in, in_bytes, parts, 5);
  if (rc == VS_OK) {
    CHECK(parts[1].dev == NULL && parts[3].dev == NULL);
    CHECK(parts[0].dev == ctx->pool.d_aux && parts[2].dev == (char *)parts[0].dev + room(a_bytes) &&
          parts[4].dev == (char *)parts[2].dev + room(b_bytes));
    CHECK(ctx->pool.d_aux_bytes >= room(a_bytes) + room(b_bytes) + room(c_bytes) && ctx->pool.d_in_bytes >= in_bytes);
    CHECK(!memcmp(ctx->pool.d_in, in, in_bytes) && !memcmp(parts[4].dev, c, c_bytes));
    memset(parts[0].dev, 5, a_bytes); /* the "kernel" */
    const int syncs = stream_syncs, copies = n_copies;
    rc = vs_host_end(ctx, launch_rc, parts, 5);
    if (launch_rc != VS_OK) CHECK(rc == launch_rc && stream_syncs == syncs + 1 && n_copies == copies && a[0] == 2 && b[0] == 3);
    else if (rc == VS_OK) CHECK(stream_syncs == syncs + 1 && n_copies == copies + 2 && a[a_bytes - 1] == 5 && b[b_bytes - 1] == (char)0xFF && c[0] == 4);
  }
  free(in);
  free(a);
  free(b);
  free(c);
  return rc;
}

/* used = 0: the context's first round makes both buffers; used = 1: a small round came before, and this one, of more
 * than the 1 MiB the buffers are grown by, frees and makes both again */
static void injection_sweep(int used)
{
  int n_calls = 0;
  for (int k = 0; n_calls == 0 || k <= n_calls; k++) { /* k = 0: the clean run that counts the calls */
    vs_ctx *ctx = new_ctx();
    if (used) CHECK(one_round(ctx, 1, VS_OK) == VS_OK && ctx->pool.d_aux_bytes == (size_t)1 << 20 && dev_live == 2);
    const size_t scale = used ? 3000 : 1;
    calls = 0;
    fail_at = k;
    failed_fn = NULL;
    const int rc = one_round(ctx, scale, VS_OK);
    fail_at = 0;
    if (k == 0) {
      /* the device set (again in each vs_pool_device that grows), hipMalloc per buffer behind its hipFree, the input
       * and two parts up, one fill, two parts down, the wait */
      CHECK(rc == VS_OK && calls == (used ? 14 : 12));
      n_calls = calls;
    } else {
      CHECK(failed_fn != NULL && rc == VS_ERR_HIP && ctx->last_hip_error == (int)hipErrorUnknown);
      CHECK(dev_live <= 2 && (ctx->pool.d_in != NULL) + (ctx->pool.d_aux != NULL) == dev_live); /* holds what is live, no more */
    }
    CHECK(one_round(ctx, scale, VS_OK) == VS_OK);
    CHECK(dev_live == 2 && ctx->pool.d_aux_bytes == (used ? (size_t)3 << 20 : (size_t)1 << 20));
    release(ctx);
  }
}

/* d_aux is asked for the sum of the parts' rounded sizes, no part forgotten and nothing added: three parts that fill
 * 1 MiB to the byte, then the same with 256 bytes more */
static void exact_fit(void)
{
  for (int over = 0; over <= 1; over++) {
    vs_ctx *ctx = new_ctx();
    const size_t a_bytes = ((size_t)1 << 20) - (over ? 256 : 512) - 3;
    char in[8] = {0}, *a = (char *)calloc(1, a_bytes), b[100] = {0}, c[100] = {0};
    if (!a) exit(2);
    VsHostPart parts[3] = {{a, a_bytes, VS_PART_UP | VS_PART_DOWN, NULL},
                           {b, sizeof(b), VS_PART_FILL_FF | VS_PART_DOWN, NULL},
                           {c, sizeof(c), VS_PART_UP, NULL}};
    CHECK(vs_host_begin(ctx, in, sizeof(in), parts, 3) == VS_OK);
    CHECK(ctx->pool.d_aux_bytes == (size_t)(1 + over) << 20);
    CHECK((char *)parts[2].dev + 256 == (char *)ctx->pool.d_aux + ((size_t)1 << 20) + (over ? 256 : 0));
    CHECK(vs_host_end(ctx, VS_OK, parts, 3) == VS_OK);
    free(a);
    release(ctx);
  }
}

static void launch_refuses(void)
{
  vs_ctx *ctx = new_ctx();
  CHECK(one_round(ctx, 1, VS_ERR_RANGE) == VS_ERR_RANGE);
  CHECK(one_round(ctx, 1, VS_ERR_NOMEM) == VS_ERR_NOMEM && ctx->last_hip_error == 0);
  CHECK(one_round(ctx, 1, VS_OK) == VS_OK);
  release(ctx);
}

int main(void)
{
  measure_calls();
  frame_calls();
  setwalk_calls();
  injection_sweep(0);
  injection_sweep(1);
  exact_fit();
  launch_refuses();
  printf("ok\n");
  return 0;
}
