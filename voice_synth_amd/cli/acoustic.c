/*
 * acoustic -- F0, jitter, shimmer and HNR of 16-bit PCM .wav files, measured on the GPU.
 *
 * The third tool of the reference's README ("acoustic: tools for measurement of jitter, shimmer, f0 and snr"), which
 * the reference never shipped.  The measurement is the library's (include/voice_synth.h, "acoustic measurement"); all
 * files of one command line go to the device in ONE vs_measure() call, each with its own length and rate.
 *
 *     acoustic [-f F0min] [-F F0max] [-m] FILE.wav ...
 *
 * stdout: a '#' line naming the columns, then one line per readable file:
 *     file F0(Hz) jitter(%) jitter(us) RAP(%) PPQ5(%) shimmer(%) shimmer(dB) APQ3(%) APQ5(%) HNR(dB) periods status
 * (NaN fields print as "nan"; status holds the VS_AC_* bits).  -m adds a line "# marks FILE: m_0 m_1 ..." after each.
 * A file that cannot be read, has a truncated header or is not 16-bit PCM (format tag 1) is named on stderr and
 * skipped; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include <math.h>

#include "cli_common.h"

static void usage(void)
{
  fprintf(stderr, "usage: acoustic [-f F0min (50 Hz)] [-F F0max (500 Hz)] [-m] FILE.wav ...\n");
}

static void field(double v, double scale, const char *fmt)
{
  if (isnan(v)) printf(" nan");
  else {
    putchar(' ');
    printf(fmt, v * scale);
  }
}

int main(int argc, char **argv)
{
  vs_measure_opts opts;
  vs_measure_defaults(&opts);
  int want_marks = 0, i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    if (strcmp(a, "-m") == 0) {
      want_marks = 1;
    } else if ((strcmp(a, "-f") == 0 || strcmp(a, "-F") == 0) && i + 1 < argc) {
      char *end = NULL;
      const double v = strtod(argv[++i], &end);
      if (!end || *end || !(v > 0.0)) {
        usage();
        return 1;
      }
      if (a[1] == 'f') opts.f0_min = (float)v;
      else opts.f0_max = (float)v;
    } else {
      usage();
      return 1;
    }
  }
  if (i >= argc) {
    usage();
    return 1;
  }
  const int nfiles = argc - i;
  VsWavRow *rows = (VsWavRow *)calloc((size_t)nfiles, sizeof(VsWavRow));
  if (!rows) return 1;
  int bad = 0, n = 0;
  int32_t maxlen = 1;
  for (int k = 0; k < nfiles; k++) {
    if (vs_cli_read_wav("acoustic", argv[i + k], &rows[n]) != 0) {
      bad = 1;
      continue;
    }
    const double tmin = floor((double)rows[n].fs / (double)opts.f0_max), tmax = ceil((double)rows[n].fs / (double)opts.f0_min);
    if (rows[n].fs <= 0 || !(tmin >= 2.0) || !(tmin < tmax) || !(tmax <= VS_AC_MAX_LAG)) { /* what vs_measure refuses */
      fprintf(stderr, "acoustic: %s: rate %d Hz with F0 %g..%g Hz is outside the measurement's lag range\n", argv[i + k],
              (int)rows[n].fs, (double)opts.f0_min, (double)opts.f0_max);
      free(rows[n].x);
      bad = 1;
      continue;
    }
    if (rows[n].len > maxlen) maxlen = rows[n].len;
    n++;
  }
  printf("# file F0_Hz jitter_%% jitter_abs_us RAP_%% PPQ5_%% shimmer_%% shimmer_dB APQ3_%% APQ5_%% HNR_dB periods status\n");
  if (n == 0) return bad ? 2 : 0;

  /* one batch: rows of maxlen samples, each with its own length and rate */
  int16_t *pcm = (int16_t *)calloc((size_t)n * (size_t)maxlen, sizeof(int16_t));
  int32_t *fs = (int32_t *)malloc((size_t)n * sizeof(int32_t));
  int32_t *len = (int32_t *)malloc((size_t)n * sizeof(int32_t));
  vs_acoustic *out = (vs_acoustic *)malloc((size_t)n * sizeof(vs_acoustic));
  size_t mpitch = 0;
  if (!pcm || !fs || !len || !out) {
    fprintf(stderr, "acoustic: out of memory\n");
    return 1;
  }
  for (int k = 0; k < n; k++) {
    memcpy(pcm + (size_t)k * maxlen, rows[k].x, (size_t)rows[k].len * sizeof(int16_t));
    fs[k] = rows[k].fs;
    len[k] = rows[k].len;
    if (want_marks && rows[k].fs > 0) { /* at most len / tmin + 1 marks */
      const double tmin = floor((double)rows[k].fs / (double)opts.f0_max);
      const size_t m = (size_t)(rows[k].len / (tmin >= 2.0 ? tmin : 2.0)) + 2;
      if (m > mpitch) mpitch = m;
    }
  }
  int32_t *marks = NULL;
  if (want_marks) {
    marks = (int32_t *)malloc((size_t)n * mpitch * sizeof(int32_t));
    if (!marks) {
      fprintf(stderr, "acoustic: out of memory\n");
      return 1;
    }
  }
  vs_ctx *ctx = NULL;
  if (vs_cli_open_ctx(&ctx) != VS_OK) return 1;
  int rc = vs_measure(ctx, &opts, pcm, (size_t)maxlen, (size_t)n, (size_t)maxlen, fs, len, out, marks, mpitch);
  if (rc != VS_OK) {
    fprintf(stderr, "acoustic: %s\n", vs_strerror(rc));
    vs_ctx_destroy(ctx);
    return 1;
  }
  for (int k = 0; k < n; k++) {
    const vs_acoustic *r = &out[k];
    printf("%s", rows[k].name);
    field(r->f0_hz, 1.0, "%.3f");
    field(r->jitter_local, 100.0, "%.4f");
    field(r->jitter_abs_s, 1e6, "%.3f");
    field(r->jitter_rap, 100.0, "%.4f");
    field(r->jitter_ppq5, 100.0, "%.4f");
    field(r->shimmer_local, 100.0, "%.4f");
    field(r->shimmer_db, 1.0, "%.4f");
    field(r->shimmer_apq3, 100.0, "%.4f");
    field(r->shimmer_apq5, 100.0, "%.4f");
    field(r->hnr_db, 1.0, "%.3f");
    printf(" %d %d\n", r->n_periods, r->status);
    if (want_marks) {
      printf("# marks %s:", rows[k].name);
      for (size_t j = 0; j < mpitch && marks[(size_t)k * mpitch + j] >= 0; j++) printf(" %d", marks[(size_t)k * mpitch + j]);
      printf("\n");
    }
  }
  vs_ctx_destroy(ctx);
  return bad ? 2 : 0;
}
