/*
 * vinverse -- inverse filtering on the GPU: a speech .wav in, the glottal flow (or the LPC residual) out.  The vocal
 * tract to undo is a vowel table, a glide between tables as vtrack -v runs it, or the LPC frames of a recording, which
 * may be the input itself.
 *
 * The filter is the library's (include/voice_synth.h, "inverse filtering").
 *
 *     vinverse -i speech.wav -o flow.wav ( -v a[,i...] | -m model.wav ) [-G] [-t hop_ms (10)] [-O order (22)]
 *              [-P] [-I [-g glottal_order (4)] [-l leak (0.99)]] [-s scale (1)] [-d de_emphasis (0)]
 *
 * -v: one table id: that table's taps, held (one set, untouched by any step-down).  Two or more ids (n of them, N
 *     samples in speech.wav): the anchors of the glide vtrack -v runs, hop = max(1, (N - 1) / (n - 1)) and offset 0, so
 *     that vinverse -v a,i -d p -s 1/g undoes vtrack -v a,i -p p -g g.
 * -m: vs_lpc of model.wav (25 ms Hamming window, hop -t, order -O, -P: with the analysis pre-emphasis) chained into the
 *     inverse on the device: each frame held for the hop around its centre, or with -G as anchors of a glide.  Frames
 *     that vs_lpc marks silent or unstable are skipped by the forward fill.
 * -I: with -m, the sets come from vs_iaif of model.wav (include/voice_synth.h, "IAIF") instead of vs_lpc: the same
 *     frames, glottal order -g and leak -l.  IAIF has no analysis pre-emphasis: -I refuses -P; -g and -l need -I.
 * -s, -d: the row's scale (1 / the gain to undo) and de-emphasis (the pre-emphasis to undo, 0..1).
 * The output file is the input's header followed by the inverse-filtered samples.
 * stdout: one line "file sets unusable clipped status" (the output file, K, and the row's vs_inverse_stat).
 * A file that cannot be read, has a truncated header or is not 16-bit PCM, or a model too short for one frame, is named
 * on stderr; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include <math.h>

#include "cli_common.h"

static void usage(void)
{
  fprintf(stderr, "usage: vinverse -i speech.wav -o flow.wav ( -v a[,i...] | -m model.wav ) [-G] [-t hop_ms (10)] "
                  "[-O order (22)] [-P] [-I [-g glottal_order (4)] [-l leak (0.99)]] [-s scale (1)] "
                  "[-d de_emphasis (0)]\n");
}

static int fail(vs_ctx *ctx, int rc)
{
  fprintf(stderr, "vinverse: %s\n", vs_strerror(rc));
  vs_ctx_destroy(ctx);
  return 1;
}

int main(int argc, char **argv)
{
  const char *in = NULL, *out = NULL, *ids = NULL, *model = NULL;
  int glide = 0, iaif = 0, iaif_args = 0;
  double scale = 1.0, rho = 0.0;
  vs_lpc_opts opts;
  vs_lpc_defaults(&opts);
  opts.n_formants = 0;
  vs_iaif_opts iopts;
  vs_iaif_defaults(&iopts);
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-G") == 0) {
      glide = 1;
    } else if (strcmp(a, "-P") == 0) {
      opts.pre_emphasis = 1;
    } else if (strcmp(a, "-I") == 0) {
      iaif = 1;
    } else if (a[0] == '-' && a[1] && !a[2] && strchr("iovm", a[1]) && i + 1 < argc) {
      const char *s = argv[++i];
      if (a[1] == 'i') in = s;
      else if (a[1] == 'o') out = s;
      else if (a[1] == 'v') ids = s;
      else model = s;
    } else if (a[0] == '-' && a[1] && !a[2] && strchr("tOsdgl", a[1]) && i + 1 < argc && number(argv[i + 1], &v)) {
      i++;
      if (a[1] == 't') {
        if (!(v > 0.0)) {
          usage();
          return 1;
        }
        opts.hop_s = v / 1000.0;
      } else if (a[1] == 'O') {
        if (v != floor(v) || v < 1 || v > VS_MAX_ORDER) {
          usage();
          return 1;
        }
        opts.order = (int32_t)v;
      } else if (a[1] == 's') {
        scale = v;
      } else if (a[1] == 'g') {
        if (v != floor(v) || v < 1 || v > VS_MAX_ORDER) {
          usage();
          return 1;
        }
        iopts.glottal_order = (int32_t)v;
        iaif_args = 1;
      } else if (a[1] == 'l') {
        if (v < 0.0 || v > 1.0) {
          usage();
          return 1;
        }
        iopts.leak = v;
        iaif_args = 1;
      } else {
        if (v < 0.0 || v > 1.0) {
          usage();
          return 1;
        }
        rho = v;
      }
    } else {
      usage();
      return 1;
    }
  }
  if (!in || !out || (!ids == !model) || (iaif && (!model || opts.pre_emphasis)) || (iaif_args && !iaif)) {
    usage();
    return 1;
  }
  if (iaif) { /* the same frames; vs_lpc_frames and vs_inverse_from_lpc below take them from opts */
    iopts.order = opts.order;
    iopts.hop_s = opts.hop_s;
    iopts.n_formants = 0;
    if (vs_iaif_lpc_opts(&iopts, &opts) != VS_OK) {
      usage();
      return 1;
    }
  }
  /* the tables of -v */
  int n_tab = 0;
  int tabs[64];
  if (ids) {
    const char *s = ids;
    for (;;) { /* id[,id]... */
      double A[VS_NCOEF];
      if (!*s || n_tab == 64 || vs_vowel_coefficients((unsigned char)*s, A) != VS_OK) {
        usage();
        return 1;
      }
      tabs[n_tab++] = (unsigned char)*s++;
      if (!*s) break;
      if (*s++ != ',') {
        usage();
        return 1;
      }
    }
  }

  VsWavRow sp, mod;
  memset(&sp, 0, sizeof(sp));
  memset(&mod, 0, sizeof(mod));
  if (vs_cli_read_wav("vinverse", in, &sp) != 0) return 2;
  if (model && vs_cli_read_wav("vinverse", model, &mod) != 0) return 2;
  /* the input's header, copied to the output verbatim (as vowel does) */
  unsigned char header[72];
  FILE *f = fopen(in, "rb");
  const size_t got = f ? fread(header, 1, sizeof(header), f) : 0;
  if (f) fclose(f);
  int32_t hfs = 0;
  int tag = 0, bits = 0;
  uint64_t data_bytes = 0;
  const int hbytes = vs_wav_header_read(header, got, &hfs, &tag, &bits, &data_bytes);
  if (hbytes < 0) return 2;
  const size_t N = (size_t)sp.len;
  if (N == 0) {
    fprintf(stderr, "vinverse: %s: no samples\n", in);
    return 2;
  }

  vs_inverse_row row;
  memset(&row, 0, sizeof(row));
  vs_inverse_stat st = {0, 0, 0, 0};
  int16_t *y = (int16_t *)calloc(N, sizeof(int16_t));
  if (!y) return 1;
  vs_ctx *ctx = NULL;
  size_t K = 0;
  int rc;
  if (ids) {
    K = (size_t)n_tab;
    double *coefs = (double *)calloc(K * VS_NCOEF, sizeof(double));
    if (!coefs) return 1;
    for (size_t k = 0; k < K; k++) vs_vowel_coefficients(tabs[k], coefs + k * VS_NCOEF);
    const long hop = K > 1 ? ((long)N - 1) / (long)(K - 1) : 1;
    row.n_sets = (int32_t)K;
    row.hop = (int32_t)(hop < 1 ? 1 : hop);
    row.offset = 0;
    row.length = (int32_t)N;
    row.scale = (float)scale;
    row.de_emphasis = (float)rho;
    if (vs_cli_open_ctx(&ctx) != VS_OK) return 1;
    rc = vs_inverse(ctx, K > 1 ? VS_TRACK_GLIDE : VS_TRACK_HOLD, VS_ORDER, sp.x, y, 1, N, &row, coefs, K, &st);
    free(coefs);
    if (rc != VS_OK) return fail(ctx, rc);
  } else {
    const int order = opts.order, mode = glide ? VS_TRACK_GLIDE : VS_TRACK_HOLD;
    int32_t nfr = 0;
    rc = vs_lpc_frames(&opts, mod.fs, mod.len, &nfr);
    if (rc == VS_OK) rc = vs_inverse_from_lpc(&opts, mod.fs, mod.len, mode, &row);
    if (rc != VS_OK) {
      fprintf(stderr, "vinverse: %s: no analysis frame (%d samples at %d Hz, %g ms window, order %d)\n", model,
              (int)mod.len, (int)mod.fs, opts.window_s * 1000.0, (int)opts.order);
      return 2;
    }
    K = (size_t)nfr;
    row.length = (int32_t)N;
    row.scale = (float)scale;
    row.de_emphasis = (float)rho;
    if (vs_cli_open_ctx(&ctx) != VS_OK) return 1;
    /* the analysis and the inverse chained on the device: the sets never come to the host */
    const size_t M = (size_t)mod.len;
    void *d_mod = NULL, *d_in = NULL, *d_out = NULL, *d_fr = NULL, *d_cf = NULL, *d_st = NULL;
    rc = vs_dev_alloc(ctx, M * sizeof(int16_t), &d_mod);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, N * sizeof(int16_t), &d_in);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, N * sizeof(int16_t), &d_out);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, K * sizeof(vs_lpc_frame), &d_fr);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, K * (size_t)(order + 1) * sizeof(double), &d_cf);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, sizeof(vs_inverse_stat), &d_st);
    if (rc == VS_OK) rc = vs_dev_upload(ctx, d_mod, mod.x, M * sizeof(int16_t));
    if (rc == VS_OK) rc = vs_dev_upload(ctx, d_in, sp.x, N * sizeof(int16_t));
    if (rc == VS_OK) rc = vs_dev_upload(ctx, d_out, y, N * sizeof(int16_t));
    if (rc == VS_OK)
      rc = iaif ? vs_iaif_launch(ctx, &iopts, (const int16_t *)d_mod, M, 1, M, &mod.fs, &mod.len, K,
                                 (vs_lpc_frame *)d_fr, NULL, (double *)d_cf, NULL)
                : vs_lpc_launch(ctx, &opts, (const int16_t *)d_mod, M, 1, M, &mod.fs, &mod.len, K, (vs_lpc_frame *)d_fr,
                                NULL, (double *)d_cf);
    if (rc == VS_OK)
      rc = vs_inverse_launch(ctx, mode, order, (const int16_t *)d_in, N, (int16_t *)d_out, N, 1, N, &row,
                             (const double *)d_cf, K, (vs_inverse_stat *)d_st);
    if (rc == VS_OK) rc = vs_dev_download(ctx, y, d_out, N * sizeof(int16_t));
    if (rc == VS_OK) rc = vs_dev_download(ctx, &st, d_st, sizeof(st));
    void *blocks[6] = {d_mod, d_in, d_out, d_fr, d_cf, d_st};
    for (int b = 0; b < 6; b++)
      if (blocks[b]) (void)vs_dev_free(ctx, blocks[b]);
    if (rc != VS_OK) return fail(ctx, rc);
  }
  vs_ctx_destroy(ctx);
  FILE *fo = fopen(out, "wb");
  if (!fo || fwrite(header, (size_t)hbytes, 1, fo) != 1 || fwrite(y, sizeof(int16_t), N, fo) != N) {
    fprintf(stderr, "vinverse: %s: cannot write\n", out);
    if (fo) fclose(fo);
    return 2;
  }
  fclose(fo);
  printf("%s %d %d %d %d\n", out, (int)K, (int)st.n_unusable, (int)st.n_clipped, (int)st.status);
  free(y);
  return 0;
}
