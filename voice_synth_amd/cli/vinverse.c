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
#include "cli_analysis.h"

static void usage(void)
{
  fprintf(stderr, "usage: vinverse -i speech.wav -o flow.wav ( -v a[,i...] | -m model.wav ) [-G] [-t hop_ms (10)] "
                  "[-O order (22)] [-P] [-I [-g glottal_order (4)] [-l leak (0.99)]] [-s scale (1)] "
                  "[-d de_emphasis (0)]\n");
}

int main(int argc, char **argv)
{
  VsCliFilter f;
  vs_cli_filter_init(&f);
  VsCliIaif iaif = {0, 0, {0}};
  vs_iaif_defaults(&iaif.opts);
  double scale = 1.0, rho = 0.0;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    double v = 0.0;
    const int shared = vs_cli_filter_arg(&f, argc, argv, &i);
    if (shared > 0) continue;
    int ok = shared == 0;
    if (ok && strcmp(a, "-P") == 0) {
      f.opts.pre_emphasis = 1;
    } else if (ok && strcmp(a, "-I") == 0) {
      iaif.on = 1;
    } else if (ok && a[0] == '-' && a[1] && !a[2] && strchr("sdgl", a[1]) && i + 1 < argc && number(argv[i + 1], &v)) {
      i++;
      if (a[1] == 's') scale = v;
      else if (a[1] == 'd') ok = v >= 0.0 && v <= 1.0;
      else ok = vs_cli_iaif_value(&iaif, a[1], v) == 0;
      if (a[1] == 'd') rho = v;
    } else {
      ok = 0;
    }
    if (!ok) {
      usage();
      return 1;
    }
  }
  /* the tables of -v: one or more; -I is of -m, and its frames are the ones vs_lpc_frames and vs_inverse_from_lpc below
   * take from f.opts */
  if (vs_cli_filter_check(&f, 1) != 0 || (iaif.on && !f.model) || vs_cli_iaif_finish(&iaif, &f.opts) != 0) {
    usage();
    return 1;
  }
  double *coefs = NULL;
  int16_t *y = NULL;
  vs_ctx *ctx = NULL;
  int status = vs_cli_filter_read("vinverse", &f);
  if (status != 0) goto done;
  const size_t N = (size_t)f.src.len;

  vs_inverse_row row;
  memset(&row, 0, sizeof(row));
  vs_inverse_stat st = {0, 0, 0, 0};
  size_t K = (size_t)f.n_tab;
  int rc;
  status = 1;
  y = (int16_t *)calloc(N, sizeof(int16_t));
  if (!y) goto done;
  if (f.ids) {
    coefs = vs_cli_filter_tables(&f);
    if (!coefs) goto done;
    row.n_sets = (int32_t)K;
    row.hop = vs_cli_filter_hop(&f);
    row.offset = 0;
    row.length = (int32_t)N;
    row.scale = (float)scale;
    row.de_emphasis = (float)rho;
    if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
    rc = vs_inverse(ctx, K > 1 ? VS_TRACK_GLIDE : VS_TRACK_HOLD, VS_ORDER, f.src.x, y, 1, N, &row, coefs, K, &st);
  } else {
    const VsWavRow *mod = &f.mod;
    const int order = f.opts.order, mode = f.glide ? VS_TRACK_GLIDE : VS_TRACK_HOLD;
    K = (size_t)vs_cli_filter_frames(&f);
    if (K < 1 || vs_inverse_from_lpc(&f.opts, mod->fs, mod->len, mode, &row) != VS_OK) {
      status = vs_cli_filter_no_frame("vinverse", &f);
      goto done;
    }
    row.length = (int32_t)N;
    row.scale = (float)scale;
    row.de_emphasis = (float)rho;
    if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
    /* the analysis and the inverse chained on the device: the sets never come to the host */
    const size_t M = (size_t)mod->len;
    void *d_mod = NULL, *d_in = NULL, *d_out = NULL, *d_fr = NULL, *d_cf = NULL, *d_st = NULL;
    rc = vs_dev_alloc(ctx, M * sizeof(int16_t), &d_mod);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, N * sizeof(int16_t), &d_in);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, N * sizeof(int16_t), &d_out);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, K * sizeof(vs_lpc_frame), &d_fr);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, K * (size_t)(order + 1) * sizeof(double), &d_cf);
    if (rc == VS_OK) rc = vs_dev_alloc(ctx, sizeof(vs_inverse_stat), &d_st);
    if (rc == VS_OK) rc = vs_dev_upload(ctx, d_mod, mod->x, M * sizeof(int16_t));
    if (rc == VS_OK) rc = vs_dev_upload(ctx, d_in, f.src.x, N * sizeof(int16_t));
    if (rc == VS_OK) rc = vs_dev_upload(ctx, d_out, y, N * sizeof(int16_t));
    if (rc == VS_OK)
      rc = iaif.on ? vs_iaif_launch(ctx, &iaif.opts, (const int16_t *)d_mod, M, 1, M, &mod->fs, &mod->len, K,
                                    (vs_lpc_frame *)d_fr, NULL, (double *)d_cf, NULL)
                   : vs_lpc_launch(ctx, &f.opts, (const int16_t *)d_mod, M, 1, M, &mod->fs, &mod->len, K,
                                   (vs_lpc_frame *)d_fr, NULL, (double *)d_cf);
    if (rc == VS_OK)
      rc = vs_inverse_launch(ctx, mode, order, (const int16_t *)d_in, N, (int16_t *)d_out, N, 1, N, &row,
                             (const double *)d_cf, K, (vs_inverse_stat *)d_st);
    if (rc == VS_OK) rc = vs_dev_download(ctx, y, d_out, N * sizeof(int16_t));
    if (rc == VS_OK) rc = vs_dev_download(ctx, &st, d_st, sizeof(st));
    void *blocks[6] = {d_mod, d_in, d_out, d_fr, d_cf, d_st};
    for (int b = 0; b < 6; b++)
      if (blocks[b]) (void)vs_dev_free(ctx, blocks[b]);
  }
  if (rc != VS_OK) {
    fprintf(stderr, "vinverse: %s\n", vs_strerror(rc));
    goto done;
  }
  status = vs_cli_write_wav("vinverse", f.out, &f.src, y, N) == 0 ? 0 : 2;
  if (status == 0) printf("%s %d %d %d %d\n", f.out, (int)K, (int)st.n_unusable, (int)st.n_clipped, (int)st.status);
done:
  vs_ctx_destroy(ctx);
  free(coefs);
  free(y);
  vs_cli_filter_free(&f);
  return status;
}
