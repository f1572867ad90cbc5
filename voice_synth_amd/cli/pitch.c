/*
 * pitch -- the pitch track of 16-bit PCM .wav files: per-frame F0, voicing and one Viterbi path, on the GPU.
 *
 * The track is the library's (include/voice_synth.h, "pitch track"); all files of one command line go to the device in
 * ONE vs_pitch() call, each with its own length and rate.
 *
 *     pitch [-f F0min] [-F F0max] [-t hop_ms] [-V voicing] [-O octave] [-J jump] [-U vuv] [-S silence_rms] [-l] FILE.wav ...
 *
 * -V, -O, -J and -U are the path's costs as fractions (Praat's 0.45, 0.01, 0.35, 0.14), rounded to Q15.
 * stdout: a '#' line naming the columns, then one line per readable file:
 *     file frames voiced segments F0_mean(Hz) F0_min(Hz) F0_max(Hz) status
 * (segments: maximal runs of voiced frames; F0 = rate / lag over the voiced frames, "nan" without one; status: the OR
 * of the frames' VS_PT_* bits).  -l adds a line "# frame FILE: start lag q status n_cand lag:q ..." per frame after each.
 * A file that cannot be read, has a truncated header, is not 16-bit PCM (format tag 1) or whose rate puts the lags or
 * the hop out of range is named on stderr and skipped; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

static void usage(void)
{
  fprintf(stderr, "usage: pitch [-f F0min (50 Hz)] [-F F0max (500 Hz)] [-t hop_ms (10)] [-V voicing (0.45)] [-O octave (0.01)] "
                  "[-J jump (0.35)] [-U vuv (0.14)] [-S silence_rms (16)] [-l] FILE.wav ...\n");
}

typedef struct {
  const vs_pitch_opts *opts;
  int32_t max_frames;
} Accept;

/* a row is accepted when vs_pitch_frames has a plan for it: one file's rate is that file's refusal, not the call's */
static int accept(const VsWavRow *r, int k, void *arg)
{
  Accept *a = (Accept *)arg;
  int32_t n = 0;
  if (vs_pitch_frames(a->opts, r->fs, r->len, &n) != VS_OK) {
    fprintf(stderr, "pitch: %s: rate %d Hz with F0 %g..%g Hz and a hop of %g ms is outside the track's range\n", r->name,
            (int)r->fs, (double)a->opts->f0_min, (double)a->opts->f0_max, a->opts->hop_s * 1000.0);
    return -1;
  }
  if (n > a->max_frames) a->max_frames = n;
  return 0;
}

static void f0(double v)
{
  if (isnan(v)) printf(" nan");
  else printf(" %.3f", v);
}

int main(int argc, char **argv)
{
  vs_pitch_opts opts;
  vs_pitch_defaults(&opts);
  int list = 0, i = 1;
  for (; i < argc && argv[i][0] == '-' && argv[i][1]; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-l") == 0) {
      list = 1;
      continue;
    }
    if (!a[1] || a[2] || !strchr("fFtVOJUS", a[1]) || i + 1 >= argc || !number(argv[i + 1], &v)) {
      usage();
      return 1;
    }
    i++;
    const int32_t q15 = (v >= 0.0 && v <= 32.0) ? (int32_t)floor(v * 32768.0 + 0.5) : -1; /* 32.0 is VS_PT_MAX_COST */
    int ok = 1;
    switch (a[1]) {
      case 'f': ok = v > 0.0; opts.f0_min = (float)v; break;
      case 'F': ok = v > 0.0; opts.f0_max = (float)v; break;
      case 't': ok = v > 0.0; opts.hop_s = v / 1000.0; break;
      case 'V': ok = q15 >= 0; opts.voicing_q = q15; break;
      case 'O': ok = q15 >= 0; opts.octave_q = q15; break;
      case 'J': ok = q15 >= 0; opts.jump_q = q15; break;
      case 'U': ok = q15 >= 0; opts.vuv_q = q15; break;
      default: ok = whole(v, 0, 32767); opts.silence_rms = (int32_t)(ok ? v : 0); break;
    }
    if (!ok) {
      usage();
      return 1;
    }
  }
  if (i >= argc) {
    usage();
    return 1;
  }
  /* one batch: rows of maxlen samples, each with its own length and rate */
  Accept acc = {&opts, 1};
  VsCliBatch b;
  int status = vs_cli_batch_load("pitch", argv + i, argc - i, accept, &acc, &b) == 0 ? 0 : 1;
  vs_pitch_frame *fr = NULL;
  vs_ctx *ctx = NULL;
  printf("# file frames voiced segments F0_mean_Hz F0_min_Hz F0_max_Hz status\n");
  if (status != 0 || b.n == 0) goto done;
  status = 1;
  const size_t fp = (size_t)acc.max_frames;
  fr = (vs_pitch_frame *)calloc((size_t)b.n * fp, sizeof(vs_pitch_frame));
  if (!fr) {
    fprintf(stderr, "pitch: out of memory\n");
    goto done;
  }
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  const int rc = vs_pitch(ctx, &opts, b.pcm, (size_t)b.maxlen, (size_t)b.n, (size_t)b.maxlen, b.fs, b.len, fp, fr);
  if (rc != VS_OK) {
    fprintf(stderr, "pitch: %s\n", vs_strerror(rc));
    goto done;
  }
  for (int k = 0; k < b.n; k++) {
    int32_t n = 0;
    vs_pitch_frames(&opts, b.fs[k], b.len[k], &n);
    const vs_pitch_frame *r = fr + (size_t)k * fp;
    int voiced = 0, segments = 0, bits = 0;
    double sum = 0.0, lo = NAN, hi = NAN;
    for (int32_t f = 0; f < n; f++) {
      bits |= r[f].status;
      if (r[f].lag <= 0) continue;
      const double hz = (double)b.fs[k] / (double)r[f].lag;
      if (f == 0 || r[f - 1].lag <= 0) segments++;
      if (voiced == 0 || hz < lo) lo = hz;
      if (voiced == 0 || hz > hi) hi = hz;
      sum += hz;
      voiced++;
    }
    printf("%s %d %d %d", b.rows[k].name, (int)n, voiced, segments);
    f0(voiced ? sum / (double)voiced : NAN);
    f0(lo);
    f0(hi);
    printf(" %d\n", bits);
    for (int32_t f = 0; list && f < n; f++) {
      printf("# frame %s: %d %d %d %d %d", b.rows[k].name, r[f].start, r[f].lag, r[f].q, r[f].status, r[f].n_cand);
      for (int c = 0; c < r[f].n_cand && c < VS_PT_MAX_CAND; c++) printf(" %d:%d", r[f].cand_lag[c], r[f].cand_q[c]);
      printf("\n");
    }
  }
  status = 0;
done:
  vs_ctx_destroy(ctx);
  free(fr);
  if (status == 0 && b.bad) status = 2;
  vs_cli_batch_free(&b);
  return status;
}
