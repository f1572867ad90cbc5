/*
 * glottal -- open, closing, speed and quasi-open quotient and the normalised amplitude quotient of 16-bit PCM .wav
 * files (glottal flows, or speech that vinverse took back to one), measured on the GPU.
 *
 * The measurement is the library's (include/voice_synth.h, "glottal parameters"); all files of one command line go to
 * the device in ONE vs_glottal() call, each with its own length and rate.
 *
 *     glottal [-f F0min] [-F F0max] [-p polarity] [-l level_open] [-L level_mid] [-c] FILE.wav ...
 *
 * stdout: a '#' line naming the columns, then one line per readable file:
 *     file OQ ClQ SQ QOQ NAQ cycles rejected status
 * (NaN fields print as "nan"; status holds the VS_GL_* bits).  -c adds one line "# cycle" per cycle after each, with the
 * twelve integers of its vs_glottal_cycle.  -p is +1 (peaks are maxima) or -1; the levels are 256ths of the amplitude.
 * A file that cannot be read, has a truncated header or is not 16-bit PCM (format tag 1) is named on stderr and
 * skipped; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

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

int main(int argc, char **argv)
{
  vs_measure_opts mopts;
  vs_glottal_opts gopts;
  vs_measure_defaults(&mopts);
  vs_glottal_defaults(&gopts);
  VsCliLag m = {"glottal", &mopts, 1, 3}; /* the marks always: three or more to a row */
  int want_cycles = 0, i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-c") == 0) {
      want_cycles = 1;
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
  const int rc = vs_glottal(ctx, &mopts, &gopts, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len, mpitch,
                            meas, marks, out, cyc, cpitch);
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
