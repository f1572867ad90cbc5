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
#include <math.h>

#include "cli_common.h"

static void usage(void)
{
  fprintf(stderr, "usage: vtrack -i flow.wav -o out.wav ( -v a,i[,u...] | -m model.wav ) [-G] [-t hop_ms (10)] "
                  "[-O order (22)] [-g gain (1)] [-p pre_emphasis (0)]\n");
}

int main(int argc, char **argv)
{
  const char *in = NULL, *out = NULL, *ids = NULL, *model = NULL;
  int glide = 0;
  double gain = 1.0, pre = 0.0;
  vs_lpc_opts opts;
  vs_lpc_defaults(&opts);
  opts.n_formants = 0;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-G") == 0) {
      glide = 1;
    } else if (a[0] == '-' && a[1] && !a[2] && strchr("iovm", a[1]) && i + 1 < argc) {
      const char *s = argv[++i];
      if (a[1] == 'i') in = s;
      else if (a[1] == 'o') out = s;
      else if (a[1] == 'v') ids = s;
      else model = s;
    } else if (a[0] == '-' && a[1] && !a[2] && strchr("tOgp", a[1]) && i + 1 < argc && number(argv[i + 1], &v)) {
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
      } else if (a[1] == 'g') {
        gain = v;
      } else {
        pre = v;
      }
    } else {
      usage();
      return 1;
    }
  }
  if (!in || !out || (!ids == !model)) {
    usage();
    return 1;
  }
  /* the anchors of -v */
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
    if (n_tab < 2) {
      usage();
      return 1;
    }
  }

  VsWavRow flow, mod;
  memset(&flow, 0, sizeof(flow));
  memset(&mod, 0, sizeof(mod));
  if (vs_cli_read_wav("vtrack", in, &flow) != 0) return 2;
  if (model && vs_cli_read_wav("vtrack", model, &mod) != 0) return 2;
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
  const size_t N = (size_t)flow.len;
  if (N == 0) {
    fprintf(stderr, "vtrack: %s: no samples\n", in);
    return 2;
  }

  vs_track_row row;
  memset(&row, 0, sizeof(row));
  int order = VS_ORDER, mode = VS_TRACK_GLIDE;
  size_t K = 0;
  double *coefs = NULL;
  vs_ctx *ctx = NULL;
  if (ids) {
    K = (size_t)n_tab;
    coefs = (double *)calloc(K * VS_NCOEF, sizeof(double));
    if (!coefs) return 1;
    for (size_t k = 0; k < K; k++) vs_vowel_coefficients(tabs[k], coefs + k * VS_NCOEF);
    const long hop = ((long)N - 1) / (long)(K - 1);
    row.n_sets = (int32_t)K;
    row.hop = (int32_t)(hop < 1 ? 1 : hop);
    row.offset = 0;
    if (vs_cli_open_ctx(&ctx) != VS_OK) return 1;
  } else {
    order = opts.order;
    mode = glide ? VS_TRACK_GLIDE : VS_TRACK_HOLD;
    int32_t nfr = 0;
    int rc = vs_lpc_frames(&opts, mod.fs, mod.len, &nfr);
    if (rc == VS_OK) rc = vs_track_from_lpc(&opts, mod.fs, mod.len, mode, &row);
    if (rc != VS_OK) {
      fprintf(stderr, "vtrack: %s: no analysis frame (%d samples at %d Hz, %g ms window, order %d)\n", model,
              (int)mod.len, (int)mod.fs, opts.window_s * 1000.0, (int)opts.order);
      return 2;
    }
    K = (size_t)nfr;
    coefs = (double *)calloc(K * (size_t)(order + 1), sizeof(double));
    vs_lpc_frame *fr = (vs_lpc_frame *)calloc(K, sizeof(vs_lpc_frame));
    if (!coefs || !fr) return 1;
    if (vs_cli_open_ctx(&ctx) != VS_OK) return 1;
    rc = vs_lpc(ctx, &opts, mod.x, (size_t)mod.len, 1, (size_t)mod.len, &mod.fs, &mod.len, K, fr, NULL, coefs);
    free(fr);
    if (rc != VS_OK) {
      fprintf(stderr, "vtrack: %s\n", vs_strerror(rc));
      vs_ctx_destroy(ctx);
      return 1;
    }
  }
  row.length = (int32_t)N;
  row.gain = (float)gain;
  row.pre_emphasis = (float)pre;

  int16_t *y = (int16_t *)calloc(N, sizeof(int16_t));
  if (!y) return 1;
  vs_track_stat st = {0, 0};
  const int rc = vs_track(ctx, mode, order, flow.x, y, 1, N, &row, coefs, NULL, K, &st);
  vs_ctx_destroy(ctx);
  if (rc != VS_OK) {
    fprintf(stderr, "vtrack: %s\n", vs_strerror(rc));
    return 1;
  }
  FILE *fo = fopen(out, "wb");
  if (!fo || fwrite(header, (size_t)hbytes, 1, fo) != 1 || fwrite(y, sizeof(int16_t), N, fo) != N) {
    fprintf(stderr, "vtrack: %s: cannot write\n", out);
    if (fo) fclose(fo);
    return 2;
  }
  fclose(fo);
  printf("%s %d %d %d\n", out, (int)K, (int)st.n_unusable, (int)st.status);
  free(y);
  free(coefs);
  return 0;
}
