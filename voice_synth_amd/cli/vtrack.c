/*
 * vtrack -- the vocal-tract filter with a coefficient track on the GPU: a glottal flow .wav in, speech out, with a tract
 * that glides between vowel tables (a diphthong) or follows the LPC frames of a recording (copy synthesis, all frames).
 *
 * The filter is the library's (include/voice_synth.h, "coefficient tracks").
 *
 *     vtrack -i flow.wav -o out.wav ( -v a,i[,u...] | -m model.wav ) [-G] [-t hop_ms (10)] [-O order (22)]
 *            [-g gain (1)] [-p pre_emphasis (0)]
 *
 * -v: two or more table ids (n of them, N samples in flow.wav) are the anchors of a glide with
 *     hop = max(1, (N - 1) / (n - 1)) and offset 0: the first table holds at sample 0, the last from sample (n - 1)*hop on.
 * -m: vs_lpc of model.wav (25 ms Hamming window, hop -t, order -O); its frames are the track, through
 *     vs_track_from_lpc: each frame held for the hop around its centre, or with -G as anchors of a glide.  Frames that
 *     vs_lpc marks silent or unstable are skipped by the track's forward fill.  No per-set gains.
 * The output file is the input's header followed by the filtered samples (as vowel writes it).
 * stdout: one line "file sets unusable status" (the output file, K, and the row's vs_track_stat).
 * A file that cannot be read, has a truncated header or is not 16-bit PCM, or a model too short for one frame, is named
 * on stderr; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

static void usage(void)
{
  fprintf(stderr, "usage: vtrack -i flow.wav -o out.wav ( -v a,i[,u...] | -m model.wav ) [-G] [-t hop_ms (10)] "
                  "[-O order (22)] [-g gain (1)] [-p pre_emphasis (0)]\n");
}

int main(int argc, char **argv)
{
  VsCliFilter f;
  vs_cli_filter_init(&f);
  double gain = 1.0, pre = 0.0;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    double v = 0.0;
    const int shared = vs_cli_filter_arg(&f, argc, argv, &i);
    if (shared > 0) continue;
    if (shared < 0 || a[0] != '-' || !a[1] || a[2] || !strchr("gp", a[1]) || i + 1 >= argc || !number(argv[++i], &v)) {
      usage();
      return 1;
    }
    if (a[1] == 'g') gain = v;
    else pre = v;
  }
  if (vs_cli_filter_check(&f, 2) != 0) { /* the anchors of -v: two or more */
    usage();
    return 1;
  }
  double *coefs = NULL;
  vs_lpc_frame *fr = NULL;
  int16_t *y = NULL;
  vs_ctx *ctx = NULL;
  int status = vs_cli_filter_read("vtrack", &f);
  if (status != 0) goto done;
  const size_t N = (size_t)f.src.len;

  vs_track_row row;
  memset(&row, 0, sizeof(row));
  int order = VS_ORDER, mode = VS_TRACK_GLIDE, rc = VS_OK;
  size_t K = (size_t)f.n_tab;
  status = 1;
  if (f.ids) {
    coefs = vs_cli_filter_tables(&f);
    row.n_sets = (int32_t)K;
    row.hop = vs_cli_filter_hop(&f);
    row.offset = 0;
  } else {
    order = f.opts.order;
    mode = f.glide ? VS_TRACK_GLIDE : VS_TRACK_HOLD;
    K = (size_t)vs_cli_filter_frames(&f);
    if (K < 1 || vs_track_from_lpc(&f.opts, f.mod.fs, f.mod.len, mode, &row) != VS_OK) {
      status = vs_cli_filter_no_frame("vtrack", &f);
      goto done;
    }
    coefs = (double *)calloc(K * (size_t)(order + 1), sizeof(double));
    fr = (vs_lpc_frame *)calloc(K, sizeof(vs_lpc_frame));
  }
  y = (int16_t *)calloc(N, sizeof(int16_t));
  if (!coefs || !y || (f.model && !fr) || vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  /* the model's sets come to the host and go back up with the flow */
  if (f.model) rc = vs_lpc(ctx, &f.opts, f.mod.x, (size_t)f.mod.len, 1, (size_t)f.mod.len, &f.mod.fs, &f.mod.len, K, fr, NULL, coefs);
  row.length = (int32_t)N;
  row.gain = (float)gain;
  row.pre_emphasis = (float)pre;
  vs_track_stat st = {0, 0};
  if (rc == VS_OK) rc = vs_track(ctx, mode, order, f.src.x, y, 1, N, &row, coefs, NULL, K, &st);
  if (rc != VS_OK) {
    fprintf(stderr, "vtrack: %s\n", vs_strerror(rc));
    goto done;
  }
  status = vs_cli_write_wav("vtrack", f.out, &f.src, y, N) == 0 ? 0 : 2;
  if (status == 0) printf("%s %d %d %d\n", f.out, (int)K, (int)st.n_unusable, (int)st.status);
done:
  vs_ctx_destroy(ctx);
  free(coefs);
  free(fr);
  free(y);
  vs_cli_filter_free(&f);
  return status;
}
