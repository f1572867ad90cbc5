/*
 * formants -- LPC analysis of 16-bit PCM .wav files on the GPU: formant frequencies and bandwidths, and the A(z) set
 * that vs_lane.A takes back (copy synthesis).
 *
 * The analysis is the library's (include/voice_synth.h, "LPC analysis"); all files of one command line go to the device
 * in ONE vs_lpc() call, each with its own length and rate.
 *
 *     formants [-o order (22)] [-w window_ms (25)] [-t hop_ms (10; 0 = centre frame)] [-n formants (5)]
 *              [-p] [-r] [-f] [-c] [-I [-g glottal_order (4)] [-l leak (0.99)]] FILE.wav ...
 *
 * stdout: a '#' line naming the columns, then one line per readable file:
 *     file frames F1_Hz B1_Hz ... Fn_Hz Bn_Hz status
 * Fi / Bi: the mean over the frames with status 0 that have at least i formants, summed in frame order ("nan" when
 * there is none); status: the VS_LPC_* bits of all frames, or-ed.  -p: analysis pre-emphasis; -r: rectangular window;
 * -f: a line "# frame FILE j start status F1 B1 ..." per frame after the file's line; -c: the centre frame only (as -t
 * 0), and a line "# coefs FILE: A0 A1 ... Ap" in %.17g, which parses back to the same doubles.
 * -I: the sets and formants of vs_iaif (include/voice_synth.h, "IAIF") instead of vs_lpc's, on the same frames, with
 * glottal order -g and leak -l.  IAIF has no analysis pre-emphasis: -I refuses -p; -g and -l need -I.
 * A file that cannot be read, has a truncated header or is not 16-bit PCM (format tag 1), or whose rate puts the window
 * out of range, is named on stderr and skipped; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

static void usage(void)
{
  fprintf(stderr, "usage: formants [-o order (22)] [-w window_ms (25)] [-t hop_ms (10; 0 = centre frame)] "
                  "[-n formants (5)] [-p] [-r] [-f] [-c] [-I [-g glottal_order (4)] [-l leak (0.99)]] FILE.wav ...\n");
}

static void field(double v)
{
  if (isnan(v)) printf(" nan");
  else printf(" %.3f", v);
}

typedef struct {
  vs_lpc_opts opts;
  int32_t *nfr, fpitch; /* every row's frames, and the most of them */
} Frames;

static int accept(const VsWavRow *r, int k, void *arg)
{
  Frames *fr = (Frames *)arg;
  if (vs_lpc_frames(&fr->opts, r->fs, r->len, &fr->nfr[k]) != VS_OK) { /* what vs_lpc refuses */
    fprintf(stderr, "formants: %s: rate %d Hz puts the %g ms window outside %d < L <= %d samples\n", r->name, (int)r->fs,
            fr->opts.window_s * 1000.0, (int)fr->opts.order, VS_LPC_MAX_WINDOW);
    return -1;
  }
  if (fr->nfr[k] > fr->fpitch) fr->fpitch = fr->nfr[k];
  return 0;
}

int main(int argc, char **argv)
{
  Frames frames = {.nfr = NULL, .fpitch = 1};
  vs_lpc_opts *const opts = &frames.opts;
  vs_lpc_defaults(opts);
  VsCliIaif iaif = {0, 0, {0}};
  vs_iaif_defaults(&iaif.opts);
  int per_frame = 0, centre = 0, i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    double v = 0.0;
    int ok = 1;
    if (strcmp(a, "-p") == 0) {
      opts->pre_emphasis = 1;
    } else if (strcmp(a, "-r") == 0) {
      opts->window = VS_LPC_RECTANGULAR;
    } else if (strcmp(a, "-f") == 0) {
      per_frame = 1;
    } else if (strcmp(a, "-c") == 0) {
      centre = 1;
    } else if (strcmp(a, "-I") == 0) {
      iaif.on = 1;
    } else if (a[1] && !a[2] && strchr("owtngl", a[1]) && i + 1 < argc && number(argv[i + 1], &v)) {
      i++;
      if (a[1] == 'o') {
        if ((ok = whole(v, 1, VS_MAX_ORDER))) opts->order = (int32_t)v;
      } else if (a[1] == 'n') {
        if ((ok = whole(v, 0, VS_LPC_MAX_FORMANTS))) opts->n_formants = (int32_t)v;
      } else if (a[1] == 'w') {
        if ((ok = v > 0.0)) opts->window_s = v / 1000.0;
      } else if (a[1] == 't') {
        if ((ok = v >= 0.0)) opts->hop_s = v / 1000.0;
      } else {
        ok = vs_cli_iaif_value(&iaif, a[1], v) == 0;
      }
    } else {
      ok = 0;
    }
    if (!ok) {
      usage();
      return 1;
    }
  }
  if (centre) opts->hop_s = 0.0;
  if (i >= argc || vs_cli_iaif_finish(&iaif, opts) != 0) { /* with -I: the same frames, which vs_lpc_frames takes from opts */
    usage();
    return 1;
  }
  const int nfiles = argc - i, nfm = opts->n_formants, nc = opts->order + 1;
  /* one batch: rows of maxlen samples, each with its own length and rate */
  VsCliBatch b;
  memset(&b, 0, sizeof(b));
  vs_lpc_frame *fr = NULL;
  double *fm = NULL, *cf = NULL;
  vs_ctx *ctx = NULL;
  int status = 1;
  frames.nfr = (int32_t *)calloc((size_t)nfiles, sizeof(int32_t));
  if (!frames.nfr) goto done;
  status = vs_cli_batch_load("formants", argv + i, nfiles, accept, &frames, &b) == 0 ? 0 : 1;
  printf("# file frames");
  for (int q = 1; q <= nfm; q++) printf(" F%d_Hz B%d_Hz", q, q);
  printf(" status\n");
  if (status != 0 || b.n == 0) goto done;
  status = 1;
  const int32_t *nfr = frames.nfr, fpitch = frames.fpitch;
  const size_t nrec = (size_t)b.n * (size_t)fpitch;
  fr = (vs_lpc_frame *)calloc(nrec, sizeof(vs_lpc_frame));
  fm = (double *)calloc(nrec * (size_t)(nfm ? 2 * nfm : 1), sizeof(double));
  if (centre) cf = (double *)calloc(nrec * (size_t)nc, sizeof(double));
  if (!fr || !fm || (centre && !cf)) {
    fprintf(stderr, "formants: out of memory\n");
    goto done;
  }
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  const int rc = iaif.on ? vs_iaif(ctx, &iaif.opts, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len,
                                   (size_t)fpitch, fr, nfm ? fm : NULL, cf, NULL)
                         : vs_lpc(ctx, opts, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len,
                                  (size_t)fpitch, fr, nfm ? fm : NULL, cf);
  if (rc != VS_OK) {
    fprintf(stderr, "formants: %s\n", vs_strerror(rc));
    goto done;
  }
  for (int k = 0; k < b.n; k++) {
    const vs_lpc_frame *r = fr + (size_t)k * fpitch;
    const double *f = fm + (size_t)k * fpitch * 2 * nfm;
    const char *name = b.rows[k].name;
    int all = 0;
    printf("%s %d", name, (int)nfr[k]);
    for (int q = 0; q < nfm; q++) {
      double sf = 0.0, sb = 0.0;
      int cnt = 0;
      for (int j = 0; j < nfr[k]; j++)
        if (r[j].status == 0 && r[j].n_formants > q) {
          sf += f[(size_t)j * 2 * nfm + 2 * q];
          sb += f[(size_t)j * 2 * nfm + 2 * q + 1];
          cnt++;
        }
      field(cnt ? sf / cnt : NAN);
      field(cnt ? sb / cnt : NAN);
    }
    for (int j = 0; j < nfr[k]; j++) all |= r[j].status;
    printf(" %d\n", all);
    if (per_frame)
      for (int j = 0; j < nfr[k]; j++) {
        printf("# frame %s %d %d %d", name, j, (int)r[j].start, (int)r[j].status);
        for (int q = 0; q < 2 * nfm; q++) field(f[(size_t)j * 2 * nfm + q]);
        printf("\n");
      }
    if (centre && nfr[k] > 0) {
      printf("# coefs %s:", name);
      for (int t = 0; t < nc; t++) printf(" %.17g", cf[(size_t)k * fpitch * nc + t]);
      printf("\n");
    }
  }
  status = 0;
done:
  vs_ctx_destroy(ctx);
  free(fr);
  free(fm);
  free(cf);
  free(frames.nfr);
  if (status == 0 && b.bad) status = 2;
  vs_cli_batch_free(&b);
  return status;
}
