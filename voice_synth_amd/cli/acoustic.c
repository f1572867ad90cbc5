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
#include "cli_analysis.h"

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
  VsCliLag m = {"acoustic", &opts, 0, 0}; /* -m: the marks, mpitch to a row */
  int i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-m") == 0) {
      m.want_marks = 1;
    } else if ((strcmp(a, "-f") == 0 || strcmp(a, "-F") == 0) && i + 1 < argc && vs_cli_real(argv[i + 1], &v) && v > 0.0) {
      i++; /* ("inf" passes, as it always has: no rate is in its lag range) */
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
  /* one batch: rows of maxlen samples, each with its own length and rate */
  VsCliBatch b;
  int status = vs_cli_batch_load("acoustic", argv + i, argc - i, vs_cli_lag_accept, &m, &b) == 0 ? 0 : 1;
  vs_acoustic *out = NULL;
  int32_t *marks = NULL;
  vs_ctx *ctx = NULL;
  printf("# file F0_Hz jitter_%% jitter_abs_us RAP_%% PPQ5_%% shimmer_%% shimmer_dB APQ3_%% APQ5_%% HNR_dB periods status\n");
  if (status != 0 || b.n == 0) goto done;
  status = 1;
  out = (vs_acoustic *)malloc((size_t)b.n * sizeof(vs_acoustic));
  if (m.want_marks) marks = (int32_t *)malloc((size_t)b.n * m.mpitch * sizeof(int32_t));
  if (!out || (m.want_marks && !marks)) {
    fprintf(stderr, "acoustic: out of memory\n");
    goto done;
  }
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  const int rc = vs_measure(ctx, &opts, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len, out, marks,
                            m.mpitch);
  if (rc != VS_OK) {
    fprintf(stderr, "acoustic: %s\n", vs_strerror(rc));
    goto done;
  }
  for (int k = 0; k < b.n; k++) {
    const vs_acoustic *r = &out[k];
    printf("%s", b.rows[k].name);
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
    if (m.want_marks) {
      printf("# marks %s:", b.rows[k].name);
      for (size_t j = 0; j < m.mpitch && marks[(size_t)k * m.mpitch + j] >= 0; j++) printf(" %d", marks[(size_t)k * m.mpitch + j]);
      printf("\n");
    }
  }
  status = 0;
done:
  vs_ctx_destroy(ctx);
  free(out);
  free(marks);
  if (status == 0 && b.bad) status = 2;
  vs_cli_batch_free(&b);
  return status;
}
