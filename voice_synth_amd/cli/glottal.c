/*
 * glottal -- open, closing, speed and quasi-open quotient and the normalised amplitude quotient of 16-bit PCM .wav
 * files (glottal flows, or speech that vinverse took back to one), measured on the GPU.
 *
 * The measurement is the library's (include/voice_synth.h, "glottal parameters"); all files of one command line go to
 * the device in ONE vs_glottal() call, each with its own length and rate.
 *
 *     glottal [-f F0min] [-F F0max] [-p polarity] [-l level_open] [-L level_mid] [-c] [-T] FILE.wav ...
 *
 * stdout: a '#' line naming the columns, then one line per readable file:
 *     file OQ ClQ SQ QOQ NAQ cycles rejected status
 * (NaN fields print as "nan"; status holds the VS_GL_* bits).  -c adds one line "# cycle" per cycle after each, with the
 * twelve integers of its vs_glottal_cycle.  -p is +1 (peaks are maxima) or -1; the levels are 256ths of the amplitude.
 * -T: the marks come from the guided walk (include/voice_synth.h, "guided marks"): the pitch track of every file, at
 * its defaults but for -f and -F, steers the walk through its longest voiced run (VS_MG_LONGEST); vs_pitch_launch,
 * vs_guided_launch and vs_glottal_launch are chained on the device.
 * A file that cannot be read, has a truncated header or is not 16-bit PCM (format tag 1) is named on stderr and
 * skipped; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

/* -T alone needs the pitch track and the guided marks: the program also links against a host side of the library that
 * lacks them (the recorded command-line trace under tests/ builds it so, and pins the usage line below), and then
 * refuses -T */
#pragma weak vs_guided_defaults
#pragma weak vs_guided_plan
#pragma weak vs_guided_launch
#pragma weak vs_pitch_defaults
#pragma weak vs_pitch_launch

static void usage(void)
{
  fprintf(stderr, "usage: glottal [-f F0min (50 Hz)] [-F F0max (500 Hz)] [-p polarity (1)] [-l level_open (26)] "
                  "[-L level_mid (128)] [-c] FILE.wav ...\n");
}

static void field(double v)
{
  if (isnan(v)) printf(" nan");
  else printf(" %.4f", v);
}

/* -T: vs_pitch_launch -> vs_guided_launch (VS_MG_LONGEST) -> vs_glottal_launch on the device; the records and, when
 * wanted, the cycles come back.  marks: the host's row block, used to fill the device's with -1 */
static int guided_chain(vs_ctx *ctx, const vs_measure_opts *mo, const vs_glottal_opts *go, const VsCliBatch *b, size_t mpitch,
                        int32_t *marks, vs_glottal_rec *out, vs_glottal_cycle *cyc, size_t cpitch)
{
  vs_guided_opts o;
  vs_pitch_opts po;
  vs_guided_defaults(&o);
  vs_pitch_defaults(&po);
  o.f0_min = po.f0_min = mo->f0_min;
  o.f0_max = po.f0_max = mo->f0_max;
  o.polarity = mo->polarity;
  o.segments = VS_MG_LONGEST;
  const size_t n = (size_t)b->n, N = (size_t)b->maxlen;
  size_t fp = 1;
  for (size_t k = 0; k < n; k++) {
    int32_t nfr = 0;
    const int rc = vs_guided_plan(&o, b->fs[k], b->len[k], NULL, NULL, NULL, &nfr, NULL);
    if (rc != VS_OK) return rc;
    if ((size_t)nfr > fp) fp = (size_t)nfr;
  }
  memset(marks, 0xFF, n * mpitch * sizeof(int32_t));
  void *d[7] = {0};
  const size_t bytes[7] = {n * N * sizeof(int16_t), n * fp * sizeof(vs_pitch_frame), n * sizeof(vs_acoustic),
                           n * mpitch * sizeof(int32_t), n * sizeof(vs_guided_rec), n * sizeof(vs_glottal_rec),
                           n * cpitch * sizeof(vs_glottal_cycle)};
  int rc = VS_OK;
  for (int k = 0; k < 7 && rc == VS_OK; k++) rc = vs_dev_alloc(ctx, bytes[k] ? bytes[k] : 1, &d[k]);
  if (rc == VS_OK) rc = vs_dev_upload(ctx, d[0], b->pcm, bytes[0]);
  if (rc == VS_OK) rc = vs_dev_upload(ctx, d[3], marks, bytes[3]);
  if (rc == VS_OK && cyc) rc = vs_dev_upload(ctx, d[6], cyc, bytes[6]);
  if (rc == VS_OK)
    rc = vs_pitch_launch(ctx, &po, (const int16_t *)d[0], N, n, N, b->fs, b->len, fp, (vs_pitch_frame *)d[1]);
  if (rc == VS_OK)
    rc = vs_guided_launch(ctx, &o, (const int16_t *)d[0], N, n, N, b->fs, b->len, (const vs_pitch_frame *)d[1], fp,
                          (vs_acoustic *)d[2], (int32_t *)d[3], mpitch, (vs_guided_rec *)d[4], NULL, 0);
  if (rc == VS_OK)
    rc = vs_glottal_launch(ctx, go, (const int16_t *)d[0], N, n, N, (const vs_acoustic *)d[2], (const int32_t *)d[3], mpitch,
                           (vs_glottal_rec *)d[5], cyc ? (vs_glottal_cycle *)d[6] : NULL, cyc ? cpitch : 0);
  if (rc == VS_OK) rc = vs_dev_download(ctx, out, d[5], bytes[5]);
  if (rc == VS_OK && cyc) rc = vs_dev_download(ctx, cyc, d[6], bytes[6]);
  for (int k = 0; k < 7; k++)
    if (d[k]) (void)vs_dev_free(ctx, d[k]);
  return rc;
}

int main(int argc, char **argv)
{
  vs_measure_opts mopts;
  vs_glottal_opts gopts;
  vs_measure_defaults(&mopts);
  vs_glottal_defaults(&gopts);
  VsCliLag m = {"glottal", &mopts, 1, 3}; /* the marks always: three or more to a row */
  int want_cycles = 0, guided = 0, i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-c") == 0) {
      want_cycles = 1;
      continue;
    }
    if (strcmp(a, "-T") == 0 && vs_guided_defaults && vs_guided_plan && vs_guided_launch && vs_pitch_defaults && vs_pitch_launch) {
      guided = 1;
      continue;
    }
    if (!a[1] || a[2] || !strchr("fFplL", a[1]) || i + 1 >= argc || !vs_cli_real(argv[++i], &v)) {
      usage();
      return 1;
    }
    int ok = 1;
    if (a[1] == 'f' || a[1] == 'F') { /* ("inf" passes, as it always has: no rate is in its lag range) */
      ok = v > 0.0;
      if (a[1] == 'f') mopts.f0_min = (float)v;
      else mopts.f0_max = (float)v;
    } else if (a[1] == 'p') {
      ok = v == 1.0 || v == -1.0;
      if (ok) mopts.polarity = gopts.polarity = (int32_t)v;
    } else {
      ok = whole(v, 0, 255);
      if (ok && a[1] == 'l') gopts.level_open = (int32_t)v;
      else if (ok) gopts.level_mid = (int32_t)v;
    }
    if (!ok) {
      usage();
      return 1;
    }
  }
  if (i >= argc || gopts.level_mid < gopts.level_open) {
    usage();
    return 1;
  }
  /* one batch: rows of maxlen samples, each with its own length and rate; every cycle of every row counts, whether its
   * record is printed or not */
  VsCliBatch b;
  int status = vs_cli_batch_load("glottal", argv + i, argc - i, vs_cli_lag_accept, &m, &b) == 0 ? 0 : 1;
  const size_t mpitch = m.mpitch, cpitch = mpitch - 2;
  vs_acoustic *meas = NULL;
  int32_t *marks = NULL;
  vs_glottal_rec *out = NULL;
  vs_glottal_cycle *cyc = NULL;
  vs_ctx *ctx = NULL;
  printf("# file OQ ClQ SQ QOQ NAQ cycles rejected status\n");
  if (status != 0 || b.n == 0) goto done;
  status = 1;
  meas = (vs_acoustic *)malloc((size_t)b.n * sizeof(vs_acoustic));
  marks = (int32_t *)malloc((size_t)b.n * mpitch * sizeof(int32_t));
  out = (vs_glottal_rec *)malloc((size_t)b.n * sizeof(vs_glottal_rec));
  if (want_cycles) cyc = (vs_glottal_cycle *)calloc((size_t)b.n * cpitch, sizeof(vs_glottal_cycle));
  if (!meas || !marks || !out || (want_cycles && !cyc)) {
    fprintf(stderr, "glottal: out of memory\n");
    goto done;
  }
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  const int rc = guided ? guided_chain(ctx, &mopts, &gopts, &b, mpitch, marks, out, cyc, cpitch)
                        : vs_glottal(ctx, &mopts, &gopts, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len,
                                     mpitch, meas, marks, out, cyc, cpitch);
  if (rc != VS_OK) {
    fprintf(stderr, "glottal: %s\n", vs_strerror(rc));
    goto done;
  }
  for (int k = 0; k < b.n; k++) {
    const vs_glottal_rec *r = &out[k];
    printf("%s", b.rows[k].name);
    field(r->oq);
    field(r->clq);
    field(r->sq);
    field(r->qoq);
    field(r->naq);
    printf(" %d %d %d\n", r->n_cycles, r->n_rejected, r->status);
    if (want_cycles) {
      const int nc = r->n_cycles + r->n_rejected;
      for (int j = 0; j < nc && (size_t)j < cpitch; j++) {
        const vs_glottal_cycle *c = &cyc[(size_t)k * cpitch + (size_t)j];
        printf("# cycle %d %d %d %d %d %d %d %d %d %d %d %d\n", c->peak, c->period, c->trough, c->amp, c->open, c->close,
               c->open_mid, c->close_mid, c->gci, c->decl, c->status, c->reserved_);
      }
    }
  }
  status = 0;
done:
  vs_ctx_destroy(ctx);
  free(meas);
  free(marks);
  free(out);
  free(cyc);
  if (status == 0 && b.bad) status = 2;
  vs_cli_batch_free(&b);
  return status;
}
