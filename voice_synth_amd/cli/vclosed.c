/*
 * vclosed -- a blind inverse filter that reaches the flow, on the GPU: a speech .wav in, the glottal flow out, with no
 * filter given.  A first pass (IAIF sets, inverse, measurement, glottal parameters) finds where every cycle closes;
 * covariance linear prediction over the closed phases alone gives the vocal tract with no source in it; the inverse with
 * that set is the flow.  All six launches are chained on the device (include/voice_synth.h, "closed-phase covariance
 * LPC").
 *
 *     vclosed -i speech.wav -o flow.wav [-O order (22)] [-f F0min (50)] [-F F0max (500)] [-p polarity (1)]
 *             [-a close|gci|peak] [-D delay (4)] [-q span_q (77)] [-w window_ms (0)] [-t hop_ms (10)]
 *             [-e first_pass_de_emphasis (0.99)] [-d de_emphasis (0)] [-s scale (1)] [-c] [-T]
 *
 * -f, -F, -p: the first pass's measurement.  Bound its pitch range so that it excludes the octave below the voice: a
 *     first pass that marks every other cycle runs the spans into the next open phase (err_over_r0 then rises a
 *     hundredfold).
 * -T: the first pass's marks come from the guided walk instead (include/voice_synth.h, "guided marks"): the residual's
 *     pitch track, at its defaults but for -f and -F, steers the walk through its longest voiced run, so that the default
 *     range is safe from the octave below.
 * -a, -D, -q: the span of a cycle: from the anchor plus delay samples, span_q / 256 of the period long.
 * -w: 0: one set from all spans of the file; else one set per frame of that many milliseconds, hop -t, each held for the
 *     hop around its centre.
 * -e: the de-emphasis of the first pass's inverse; -d, -s: the de-emphasis and scale of the inverse that writes the flow.
 * -c: also prints every set, "# set a_0 ... a_p" in %.17g, before the line.
 * stdout: one line "file sets unusable clipped spans equations err_over_r0 status": the output file, the number of
 * sets, n_unusable and n_clipped of the inverse, the spans pooled and their equations summed over the sets, the largest
 * err / r0 of the sets that have one (%.3e, or nan) and the OR of the sets' status words.
 * A file that cannot be read, has a truncated header or is not 16-bit PCM, has no samples or a rate outside the
 * measurement's lag range is named on stderr; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

static void usage(void)
{
  fprintf(stderr, "usage: vclosed -i speech.wav -o flow.wav [-O order (22)] [-f F0min (50)] [-F F0max (500)] "
                  "[-p polarity (1)] [-a close|gci|peak] [-D delay (4)] [-q span_q (77)] [-w window_ms (0)] "
                  "[-t hop_ms (10)] [-e first_pass_de_emphasis (0.99)] [-d de_emphasis (0)] [-s scale (1)] [-c] [-T]\n");
}

int main(int argc, char **argv)
{
  const char *in = NULL, *out = NULL;
  vs_cplpc_opts co;
  vs_iaif_opts io;
  vs_measure_opts mo;
  vs_glottal_opts go;
  vs_cplpc_defaults(&co);
  vs_iaif_defaults(&io);
  vs_measure_defaults(&mo);
  vs_glottal_defaults(&go);
  co.n_formants = 0;
  io.n_formants = 0;
  double rho1 = 0.99, rho = 0.0, scale = 1.0;
  int print_sets = 0, guided = 0;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    double v = 0.0;
    int ok = 1;
    if (strcmp(a, "-c") == 0) {
      print_sets = 1;
    } else if (strcmp(a, "-T") == 0) {
      guided = 1;
    } else if (a[0] == '-' && a[1] && !a[2] && strchr("ioa", a[1]) && i + 1 < argc) {
      const char *s = argv[++i];
      if (a[1] == 'i') in = s;
      else if (a[1] == 'o') out = s;
      else if (strcmp(s, "close") == 0) co.anchor = VS_CP_ANCHOR_CLOSE;
      else if (strcmp(s, "gci") == 0) co.anchor = VS_CP_ANCHOR_GCI;
      else if (strcmp(s, "peak") == 0) co.anchor = VS_CP_ANCHOR_PEAK;
      else ok = 0;
    } else if (a[0] == '-' && a[1] && !a[2] && strchr("OfFpDqwteds", a[1]) && i + 1 < argc && number(argv[i + 1], &v)) {
      i++;
      switch (a[1]) {
      case 'O': ok = whole(v, 1, VS_MAX_ORDER); co.order = (int32_t)v; break;
      case 'f': ok = v > 0.0; mo.f0_min = (float)v; break;
      case 'F': ok = v > 0.0; mo.f0_max = (float)v; break;
      case 'p': ok = v == 1.0 || v == -1.0; mo.polarity = go.polarity = (int32_t)v; break;
      case 'D': ok = whole(v, -32768, 32767); co.delay = (int32_t)v; break;
      case 'q': ok = whole(v, 1, 256); co.span_q = (int32_t)v; break;
      case 'w': ok = v >= 0.0; co.window_s = v / 1000.0; break;
      case 't': ok = v > 0.0; co.hop_s = v / 1000.0; break;
      case 'e': ok = v >= 0.0 && v <= 1.0; rho1 = v; break;
      case 'd': ok = v >= 0.0 && v <= 1.0; rho = v; break;
      default: scale = v; break;
      }
    } else {
      ok = 0;
    }
    if (!ok) {
      usage();
      return 1;
    }
  }
  vs_lpc_opts ilo, clo;
  io.order = co.order;
  if (io.glottal_order > io.order) io.glottal_order = io.order;
  if (!in || !out || vs_iaif_lpc_opts(&io, &ilo) != VS_OK || vs_cplpc_lpc_opts(&co, &clo) != VS_OK) {
    usage();
    return 1;
  }

  VsWavRow src;
  memset(&src, 0, sizeof(src));
  vs_ctx *ctx = NULL;
  int16_t *y = NULL;
  vs_lpc_frame *fr = NULL;
  double *cf = NULL;
  int32_t *cnt = NULL;
  int status = 2;
  if (vs_cli_read_wav("vclosed", in, &src) != 0) goto done;
  if (src.len == 0) {
    fprintf(stderr, "vclosed: %s: no samples\n", in);
    goto done;
  }
  VsCliLag lag = {"vclosed", &mo, 1, 1};
  if (vs_cli_lag_accept(&src, 0, &lag) != 0) goto done;
  const size_t N = (size_t)src.len, mp = lag.mpitch, cp = lag.mpitch, P1 = (size_t)co.order + 1;

  /* the first pass's frames and its inverse row; the estimate's frames and the row that plays them */
  int32_t ifr = 0, cfr = 0;
  vs_inverse_row row1, row2;
  if (vs_lpc_frames(&ilo, src.fs, src.len, &ifr) != VS_OK || ifr < 1 ||
      vs_inverse_from_lpc(&ilo, src.fs, src.len, VS_TRACK_HOLD, &row1) != VS_OK ||
      vs_cplpc_frames(&co, src.fs, src.len, &cfr) != VS_OK || cfr < 1) {
    fprintf(stderr, "vclosed: %s: no analysis frame (%d samples at %d Hz, order %d)\n", in, (int)src.len, (int)src.fs,
            (int)co.order);
    goto done;
  }
  if (co.window_s > 0.0) {
    if (vs_inverse_from_lpc(&clo, src.fs, src.len, VS_TRACK_HOLD, &row2) != VS_OK) goto done;
  } else {
    memset(&row2, 0, sizeof(row2));
    row2.n_sets = 1;
    row2.hop = 1;
    row2.offset = 0;
    row2.length = src.len;
  }
  row1.scale = row2.scale = (float)scale;
  row1.de_emphasis = (float)rho1;
  row2.de_emphasis = (float)rho;
  const size_t K1 = (size_t)ifr, K = (size_t)cfr;
  /* -T: the residual's pitch track and the guided walk through its longest run */
  vs_guided_opts gdo;
  vs_pitch_opts pto;
  vs_guided_defaults(&gdo);
  vs_pitch_defaults(&pto);
  gdo.f0_min = pto.f0_min = mo.f0_min;
  gdo.f0_max = pto.f0_max = mo.f0_max;
  gdo.polarity = mo.polarity;
  gdo.segments = VS_MG_LONGEST;
  int32_t pfr = 0;
  if (guided && vs_guided_plan(&gdo, src.fs, src.len, NULL, NULL, NULL, &pfr, NULL) != VS_OK) goto done;
  const size_t FP = pfr > 0 ? (size_t)pfr : 1;

  status = 1;
  y = (int16_t *)calloc(N, sizeof(int16_t));
  fr = (vs_lpc_frame *)calloc(K, sizeof(vs_lpc_frame));
  cf = (double *)calloc(K * P1, sizeof(double));
  cnt = (int32_t *)calloc(K * 2, sizeof(int32_t));
  if (!y || !fr || !cf || !cnt) goto done;
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  void *d[12] = {0};
  const size_t bytes[12] = {N * sizeof(int16_t), K1 * sizeof(vs_lpc_frame), K1 * P1 * sizeof(double), N * sizeof(int16_t),
                            sizeof(vs_acoustic), mp * sizeof(int32_t), sizeof(vs_glottal_rec),
                            cp * sizeof(vs_glottal_cycle), K * sizeof(vs_lpc_frame), K * P1 * sizeof(double),
                            K * 2 * sizeof(int32_t), N * sizeof(int16_t)};
  void *d_st = NULL, *d_ptf = NULL, *d_grec = NULL;
  vs_inverse_stat st = {0, 0, 0, 0};
  int rc = vs_dev_alloc(ctx, sizeof(st), &d_st);
  if (rc == VS_OK && guided) rc = vs_dev_alloc(ctx, FP * sizeof(vs_pitch_frame), &d_ptf);
  if (rc == VS_OK && guided) rc = vs_dev_alloc(ctx, sizeof(vs_guided_rec), &d_grec);
  for (int b = 0; b < 12 && rc == VS_OK; b++) rc = vs_dev_alloc(ctx, bytes[b], &d[b]);
  if (rc == VS_OK) rc = vs_dev_upload(ctx, d[0], src.x, N * sizeof(int16_t));
  if (rc == VS_OK) rc = vs_dev_upload(ctx, d[3], y, N * sizeof(int16_t));
  if (rc == VS_OK) rc = vs_dev_upload(ctx, d[11], y, N * sizeof(int16_t));
  /* the chain: nothing of it comes to the host but the flow, the sets and their records */
  if (rc == VS_OK)
    rc = vs_iaif_launch(ctx, &io, (const int16_t *)d[0], N, 1, N, &src.fs, &src.len, K1, (vs_lpc_frame *)d[1], NULL,
                        (double *)d[2], NULL);
  if (rc == VS_OK)
    rc = vs_inverse_launch(ctx, VS_TRACK_HOLD, co.order, (const int16_t *)d[0], N, (int16_t *)d[3], N, 1, N, &row1,
                           (const double *)d[2], K1, NULL);
  if (rc == VS_OK && guided)
    rc = vs_pitch_launch(ctx, &pto, (const int16_t *)d[3], N, 1, N, &src.fs, &src.len, FP, (vs_pitch_frame *)d_ptf);
  if (rc == VS_OK && guided)
    rc = vs_guided_launch(ctx, &gdo, (const int16_t *)d[3], N, 1, N, &src.fs, &src.len, (const vs_pitch_frame *)d_ptf, FP,
                          (vs_acoustic *)d[4], (int32_t *)d[5], mp, (vs_guided_rec *)d_grec, NULL, 0);
  if (rc == VS_OK && !guided)
    rc = vs_measure_launch(ctx, &mo, (const int16_t *)d[3], N, 1, N, &src.fs, &src.len, (vs_acoustic *)d[4],
                           (int32_t *)d[5], mp);
  if (rc == VS_OK)
    rc = vs_glottal_launch(ctx, &go, (const int16_t *)d[3], N, 1, N, (const vs_acoustic *)d[4], (const int32_t *)d[5], mp,
                           (vs_glottal_rec *)d[6], (vs_glottal_cycle *)d[7], cp);
  if (rc == VS_OK)
    rc = vs_cplpc_launch(ctx, &co, (const int16_t *)d[0], N, 1, N, &src.fs, &src.len, (const vs_glottal_rec *)d[6],
                         (const vs_glottal_cycle *)d[7], cp, K, (vs_lpc_frame *)d[8], NULL, (double *)d[9],
                         (int32_t *)d[10]);
  if (rc == VS_OK)
    rc = vs_inverse_launch(ctx, VS_TRACK_HOLD, co.order, (const int16_t *)d[0], N, (int16_t *)d[11], N, 1, N, &row2,
                           (const double *)d[9], K, (vs_inverse_stat *)d_st);
  if (rc == VS_OK) rc = vs_dev_download(ctx, y, d[11], N * sizeof(int16_t));
  if (rc == VS_OK) rc = vs_dev_download(ctx, fr, d[8], K * sizeof(vs_lpc_frame));
  if (rc == VS_OK) rc = vs_dev_download(ctx, cf, d[9], K * P1 * sizeof(double));
  if (rc == VS_OK) rc = vs_dev_download(ctx, cnt, d[10], K * 2 * sizeof(int32_t));
  if (rc == VS_OK) rc = vs_dev_download(ctx, &st, d_st, sizeof(st));
  for (int b = 0; b < 12; b++)
    if (d[b]) (void)vs_dev_free(ctx, d[b]);
  if (d_st) (void)vs_dev_free(ctx, d_st);
  if (d_ptf) (void)vs_dev_free(ctx, d_ptf);
  if (d_grec) (void)vs_dev_free(ctx, d_grec);
  if (rc != VS_OK) {
    fprintf(stderr, "vclosed: %s\n", vs_strerror(rc));
    goto done;
  }
  status = vs_cli_write_wav("vclosed", out, &src, y, N) == 0 ? 0 : 2;
  if (status == 0) {
    long spans = 0, eqs = 0;
    int all = 0;
    double worst = NAN;
    for (size_t k = 0; k < K; k++) {
      spans += cnt[2 * k];
      eqs += cnt[2 * k + 1];
      all |= fr[k].status;
      const double q = fr[k].r0 != 0.0 ? fr[k].err / fr[k].r0 : NAN;
      if (!isnan(q) && !(q <= worst)) worst = q;
      if (print_sets) {
        printf("# set");
        for (size_t j = 0; j < P1; j++) printf(" %.17g", cf[k * P1 + j]);
        printf("\n");
      }
    }
    char qs[32];
    if (isnan(worst)) snprintf(qs, sizeof(qs), "nan");
    else snprintf(qs, sizeof(qs), "%.3e", worst);
    printf("%s %d %d %d %ld %ld %s %d\n", out, (int)K, (int)st.n_unusable, (int)st.n_clipped, spans, eqs, qs, all);
  }
done:
  vs_ctx_destroy(ctx);
  free(y);
  free(fr);
  free(cf);
  free(cnt);
  free(src.x);
  return status;
}
