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
#include <math.h>

#include "cli_common.h"

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

int main(int argc, char **argv)
{
  vs_lpc_opts opts;
  vs_lpc_defaults(&opts);
  vs_iaif_opts iopts;
  vs_iaif_defaults(&iopts);
  int per_frame = 0, centre = 0, iaif = 0, iaif_args = 0, i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-p") == 0) {
      opts.pre_emphasis = 1;
    } else if (strcmp(a, "-r") == 0) {
      opts.window = VS_LPC_RECTANGULAR;
    } else if (strcmp(a, "-f") == 0) {
      per_frame = 1;
    } else if (strcmp(a, "-c") == 0) {
      centre = 1;
    } else if (strcmp(a, "-I") == 0) {
      iaif = 1;
    } else if (a[1] && !a[2] && strchr("owtngl", a[1]) && i + 1 < argc && number(argv[i + 1], &v)) {
      i++;
      if (a[1] == 'o') {
        if (v != floor(v) || v < 1 || v > VS_MAX_ORDER) {
          usage();
          return 1;
        }
        opts.order = (int32_t)v;
      } else if (a[1] == 'n') {
        if (v != floor(v) || v < 0 || v > VS_LPC_MAX_FORMANTS) {
          usage();
          return 1;
        }
        opts.n_formants = (int32_t)v;
      } else if (a[1] == 'g') {
        if (v != floor(v) || v < 1 || v > VS_MAX_ORDER) {
          usage();
          return 1;
        }
        iopts.glottal_order = (int32_t)v;
        iaif_args = 1;
      } else if (a[1] == 'l') {
        if (!(v >= 0.0 && v <= 1.0)) {
          usage();
          return 1;
        }
        iopts.leak = v;
        iaif_args = 1;
      } else if (a[1] == 'w') {
        if (!(v > 0.0)) {
          usage();
          return 1;
        }
        opts.window_s = v / 1000.0;
      } else {
        if (!(v >= 0.0)) {
          usage();
          return 1;
        }
        opts.hop_s = v / 1000.0;
      }
    } else {
      usage();
      return 1;
    }
  }
  if (centre) opts.hop_s = 0.0;
  if (i >= argc || (iaif && opts.pre_emphasis) || (iaif_args && !iaif)) {
    usage();
    return 1;
  }
  if (iaif) { /* the same frames: vs_lpc_frames below takes them from opts */
    iopts.order = opts.order;
    iopts.window = opts.window;
    iopts.n_formants = opts.n_formants;
    iopts.window_s = opts.window_s;
    iopts.hop_s = opts.hop_s;
    if (vs_iaif_lpc_opts(&iopts, &opts) != VS_OK) {
      usage();
      return 1;
    }
  }
  const int nfiles = argc - i, nfm = opts.n_formants, nc = opts.order + 1;
  VsWavRow *rows = (VsWavRow *)calloc((size_t)nfiles, sizeof(VsWavRow));
  int32_t *nfr = (int32_t *)calloc((size_t)nfiles, sizeof(int32_t));
  if (!rows || !nfr) return 1;
  int bad = 0, n = 0;
  int32_t maxlen = 1, fpitch = 1;
  for (int k = 0; k < nfiles; k++) {
    if (vs_cli_read_wav("formants", argv[i + k], &rows[n]) != 0) {
      bad = 1;
      continue;
    }
    if (vs_lpc_frames(&opts, rows[n].fs, rows[n].len, &nfr[n]) != VS_OK) { /* what vs_lpc refuses */
      fprintf(stderr, "formants: %s: rate %d Hz puts the %g ms window outside %d < L <= %d samples\n", argv[i + k],
              (int)rows[n].fs, opts.window_s * 1000.0, (int)opts.order, VS_LPC_MAX_WINDOW);
      free(rows[n].x);
      bad = 1;
      continue;
    }
    if (rows[n].len > maxlen) maxlen = rows[n].len;
    if (nfr[n] > fpitch) fpitch = nfr[n];
    n++;
  }
  printf("# file frames");
  for (int q = 1; q <= nfm; q++) printf(" F%d_Hz B%d_Hz", q, q);
  printf(" status\n");
  if (n == 0) return bad ? 2 : 0;

  /* one batch: rows of maxlen samples, each with its own length and rate */
  const size_t nrec = (size_t)n * (size_t)fpitch;
  int16_t *pcm = (int16_t *)calloc((size_t)n * (size_t)maxlen, sizeof(int16_t));
  int32_t *fs = (int32_t *)malloc((size_t)n * sizeof(int32_t));
  int32_t *len = (int32_t *)malloc((size_t)n * sizeof(int32_t));
  vs_lpc_frame *fr = (vs_lpc_frame *)calloc(nrec, sizeof(vs_lpc_frame));
  double *fm = (double *)calloc(nrec * (size_t)(nfm ? 2 * nfm : 1), sizeof(double));
  double *cf = centre ? (double *)calloc(nrec * (size_t)nc, sizeof(double)) : NULL;
  if (!pcm || !fs || !len || !fr || !fm || (centre && !cf)) {
    fprintf(stderr, "formants: out of memory\n");
    return 1;
  }
  for (int k = 0; k < n; k++) {
    memcpy(pcm + (size_t)k * maxlen, rows[k].x, (size_t)rows[k].len * sizeof(int16_t));
    fs[k] = rows[k].fs;
    len[k] = rows[k].len;
  }
  vs_ctx *ctx = NULL;
  if (vs_cli_open_ctx(&ctx) != VS_OK) return 1;
  int rc = iaif ? vs_iaif(ctx, &iopts, pcm, (size_t)maxlen, (size_t)n, (size_t)maxlen, fs, len, (size_t)fpitch, fr,
                          nfm ? fm : NULL, cf, NULL)
                : vs_lpc(ctx, &opts, pcm, (size_t)maxlen, (size_t)n, (size_t)maxlen, fs, len, (size_t)fpitch, fr,
                         nfm ? fm : NULL, cf);
  if (rc != VS_OK) {
    fprintf(stderr, "formants: %s\n", vs_strerror(rc));
    vs_ctx_destroy(ctx);
    return 1;
  }
  for (int k = 0; k < n; k++) {
    const vs_lpc_frame *r = fr + (size_t)k * fpitch;
    const double *f = fm + (size_t)k * fpitch * 2 * nfm;
    int status = 0;
    printf("%s %d", rows[k].name, (int)nfr[k]);
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
    for (int j = 0; j < nfr[k]; j++) status |= r[j].status;
    printf(" %d\n", status);
    if (per_frame)
      for (int j = 0; j < nfr[k]; j++) {
        printf("# frame %s %d %d %d", rows[k].name, j, (int)r[j].start, (int)r[j].status);
        for (int q = 0; q < 2 * nfm; q++) field(f[(size_t)j * 2 * nfm + q]);
        printf("\n");
      }
    if (centre && nfr[k] > 0) {
      printf("# coefs %s:", rows[k].name);
      for (int t = 0; t < nc; t++) printf(" %.17g", cf[(size_t)k * fpitch * nc + t]);
      printf("\n");
    }
  }
  vs_ctx_destroy(ctx);
  return bad ? 2 : 0;
}
