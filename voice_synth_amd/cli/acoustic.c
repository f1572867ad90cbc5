/*
 * acoustic -- F0, jitter, shimmer and HNR of 16-bit PCM .wav files, measured on the GPU.
 *
 * The third tool of the reference's README ("acoustic: tools for measurement of jitter, shimmer, f0 and snr"), which
 * the reference never shipped.  The measurement is the library's (include/voice_synth.h, "acoustic measurement"); all
 * files of one command line go to the device in ONE vs_measure() call, each with its own length and rate.
 *
 *     acoustic [-f F0min] [-F F0max] [-m] [-T] FILE.wav ...
 *
 * stdout: a '#' line naming the columns, then one line per readable file:
 *     file F0(Hz) jitter(%) jitter(us) RAP(%) PPQ5(%) shimmer(%) shimmer(dB) APQ3(%) APQ5(%) HNR(dB) periods status
 * (NaN fields print as "nan"; status holds the VS_AC_* bits).  -m adds a line "# marks FILE: m_0 m_1 ..." after each.
 * -T: the guided marks (include/voice_synth.h, "guided marks"): the pitch track of every file, at its defaults but for
 * -f and -F, steers the walk through all its voiced runs (vs_guided(), VS_MG_ALL); two columns are added, segments and
 * voiced_frames, and -m lists the marks of all runs one behind the other.
 * A file that cannot be read, has a truncated header or is not 16-bit PCM (format tag 1) is named on stderr and
 * skipped; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

/* -T alone needs the guided marks: the program also links against a host side of the library that lacks them (the
 * recorded command-line trace under tests/ builds it so, and pins the usage line below), and then refuses -T */
#pragma weak vs_guided_defaults
#pragma weak vs_guided_plan
#pragma weak vs_guided

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
  int i = 1, guided = 0;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-m") == 0) {
      m.want_marks = 1;
    } else if (strcmp(a, "-T") == 0 && vs_guided_defaults && vs_guided_plan && vs_guided) {
      guided = 1;
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
  vs_guided_rec *grec = NULL;
  vs_ctx *ctx = NULL;
  printf("# file F0_Hz jitter_%% jitter_abs_us RAP_%% PPQ5_%% shimmer_%% shimmer_dB APQ3_%% APQ5_%% HNR_dB periods status%s\n",
         guided ? " segments voiced_frames" : "");
  if (status != 0 || b.n == 0) goto done;
  status = 1;
  /* -T: the frames of the longest track; every run may end on one mark more than its periods */
  vs_guided_opts gopts;
  memset(&gopts, 0, sizeof(gopts));
  if (guided) vs_guided_defaults(&gopts);
  gopts.f0_min = opts.f0_min;
  gopts.f0_max = opts.f0_max;
  size_t fpitch = 1;
  for (int k = 0; guided && k < b.n; k++) {
    int32_t nfr = 0;
    if (vs_guided_plan(&gopts, b.fs[k], b.len[k], NULL, NULL, NULL, &nfr, NULL) == VS_OK && (size_t)nfr > fpitch) fpitch = (size_t)nfr;
  }
  if (guided && m.want_marks) m.mpitch += fpitch;
  out = (vs_acoustic *)malloc((size_t)b.n * sizeof(vs_acoustic));
  if (m.want_marks) marks = (int32_t *)malloc((size_t)b.n * m.mpitch * sizeof(int32_t));
  if (guided) grec = (vs_guided_rec *)malloc((size_t)b.n * sizeof(vs_guided_rec));
  if (!out || (m.want_marks && !marks) || (guided && !grec)) {
    fprintf(stderr, "acoustic: out of memory\n");
    goto done;
  }
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  const int rc = guided ? vs_guided(ctx, &gopts, NULL, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len,
                                    fpitch, NULL, out, marks, m.mpitch, grec, NULL, 0)
                        : vs_measure(ctx, &opts, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len, out,
                                     marks, m.mpitch);
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
    printf(" %d %d", r->n_periods, r->status);
    if (guided) printf(" %d %d", grec[k].n_segments, grec[k].n_frames_walked);
    printf("\n");
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
  free(grec);
  if (status == 0 && b.bad) status = 2;
  vs_cli_batch_free(&b);
  return status;
}
