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
#include <math.h>

#include "cli_common.h"

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
  int want_cycles = 0, i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    if (strcmp(a, "-c") == 0) {
      want_cycles = 1;
    } else if (a[1] && !a[2] && strchr("fFplL", a[1]) && i + 1 < argc) {
      char *end = NULL;
      const double v = strtod(argv[++i], &end);
      if (!end || *end || end == argv[i]) {
        usage();
        return 1;
      }
      if (a[1] == 'f' || a[1] == 'F') {
        if (!(v > 0.0)) {
          usage();
          return 1;
        }
        if (a[1] == 'f') mopts.f0_min = (float)v;
        else mopts.f0_max = (float)v;
      } else if (a[1] == 'p') {
        if (v != 1.0 && v != -1.0) {
          usage();
          return 1;
        }
        mopts.polarity = gopts.polarity = (int32_t)v;
      } else {
        if (!(v >= 0.0 && v <= 255.0) || v != floor(v)) {
          usage();
          return 1;
        }
        if (a[1] == 'l') gopts.level_open = (int32_t)v;
        else gopts.level_mid = (int32_t)v;
      }
    } else {
      usage();
      return 1;
    }
  }
  if (i >= argc || gopts.level_mid < gopts.level_open) {
    usage();
    return 1;
  }
  const int nfiles = argc - i;
  VsWavRow *rows = (VsWavRow *)calloc((size_t)nfiles, sizeof(VsWavRow));
  if (!rows) return 1;
  int bad = 0, n = 0;
  int32_t maxlen = 1;
  size_t mpitch = 3;
  for (int k = 0; k < nfiles; k++) {
    if (vs_cli_read_wav("glottal", argv[i + k], &rows[n]) != 0) {
      bad = 1;
      continue;
    }
    const double tmin = floor((double)rows[n].fs / (double)mopts.f0_max), tmax = ceil((double)rows[n].fs / (double)mopts.f0_min);
    if (rows[n].fs <= 0 || !(tmin >= 2.0) || !(tmin < tmax) || !(tmax <= VS_AC_MAX_LAG)) { /* what vs_measure refuses */
      fprintf(stderr, "glottal: %s: rate %d Hz with F0 %g..%g Hz is outside the measurement's lag range\n", argv[i + k],
              (int)rows[n].fs, (double)mopts.f0_min, (double)mopts.f0_max);
      free(rows[n].x);
      bad = 1;
      continue;
    }
    if (rows[n].len > maxlen) maxlen = rows[n].len;
    const size_t m = (size_t)(rows[n].len / tmin) + 2; /* at most len / tmin + 1 marks */
    if (m > mpitch) mpitch = m;
    n++;
  }
  printf("# file OQ ClQ SQ QOQ NAQ cycles rejected status\n");
  if (n == 0) return bad ? 2 : 0;

  /* one batch: rows of maxlen samples, each with its own length and rate; every cycle of every row counts, whether its
   * record is printed or not */
  const size_t cpitch = mpitch - 2;
  int16_t *pcm = (int16_t *)calloc((size_t)n * (size_t)maxlen, sizeof(int16_t));
  int32_t *fs = (int32_t *)malloc((size_t)n * sizeof(int32_t));
  int32_t *len = (int32_t *)malloc((size_t)n * sizeof(int32_t));
  vs_acoustic *meas = (vs_acoustic *)malloc((size_t)n * sizeof(vs_acoustic));
  int32_t *marks = (int32_t *)malloc((size_t)n * mpitch * sizeof(int32_t));
  vs_glottal_rec *out = (vs_glottal_rec *)malloc((size_t)n * sizeof(vs_glottal_rec));
  vs_glottal_cycle *cyc = want_cycles ? (vs_glottal_cycle *)calloc((size_t)n * cpitch, sizeof(vs_glottal_cycle)) : NULL;
  if (!pcm || !fs || !len || !meas || !marks || !out || (want_cycles && !cyc)) {
    fprintf(stderr, "glottal: out of memory\n");
    return 1;
  }
  for (int k = 0; k < n; k++) {
    memcpy(pcm + (size_t)k * maxlen, rows[k].x, (size_t)rows[k].len * sizeof(int16_t));
    fs[k] = rows[k].fs;
    len[k] = rows[k].len;
  }
  vs_ctx *ctx = NULL;
  if (vs_cli_open_ctx(&ctx) != VS_OK) return 1;
  int rc = vs_glottal(ctx, &mopts, &gopts, pcm, (size_t)maxlen, (size_t)n, (size_t)maxlen, fs, len, mpitch, meas, marks,
                      out, cyc, cpitch);
  if (rc != VS_OK) {
    fprintf(stderr, "glottal: %s\n", vs_strerror(rc));
    vs_ctx_destroy(ctx);
    return 1;
  }
  for (int k = 0; k < n; k++) {
    const vs_glottal_rec *r = &out[k];
    printf("%s", rows[k].name);
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
  vs_ctx_destroy(ctx);
  return bad ? 2 : 0;
}
