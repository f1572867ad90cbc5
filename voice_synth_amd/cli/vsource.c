/*
 * vsource -- a glottal source that moves, on the GPU: flowgen_shimmer's pulses on an F0 contour that comes from a
 * recording's pitch track or from a few anchors.
 *
 * The source is the library's (include/voice_synth.h, "source track").
 *
 *     vsource -o flow.wav ( -M model.wav [-A] | -C f0,f0[,f0...] ) [-L F0min (50)] [-H F0max (500)] [-T hop_ms (10)]
 *             [-S seed] [flowgen_shimmer's -r -d -j -s -c -k -z -n -a -l]
 *
 * Its own letters are capitals and are told from flowgen_shimmer's by their case; -f and -g are not accepted (the
 * contour is the F0, and there is no glottal formant to hold it against).
 * -M: vs_pitch of model.wav (range -L..-H, hop -T) gives the period of every frame, through vs_strack_from_pitch; the
 *     rate and the length are the model's (-r and -d play no part), the output file has the model's header.
 *     -A adds the amplitude track amp_f = floor(a * sqrt((double)r0_f / (double)max_f r0_f) + 0.5), a the value of -a.
 * -C: two or more anchors in Hz, spread evenly over the -d seconds (N samples): frames of hop H from sample 0, the
 *     centre of frame f at c = min(f*H + H/2, N), F0_f linear between the anchors at u = c * (n - 1) / N, period
 *     (int)(fs / F0_f).  A period outside floor(fs/F0max)..ceil(fs/F0min) is unvoiced.
 * -S: the seed of the draws; else VS_SEED, else the clock, as flowgen_shimmer.
 * stdout: one line "file frames voiced cycles resets status" (the output file, the frames of the track, how many of them
 * are voiced, and the row's vs_strack_stat).
 * A file that cannot be read, has a truncated header or is not 16-bit PCM, or a model without a frame, is named on
 * stderr; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

static void usage(void)
{
  fprintf(stderr, "usage: vsource -o flow.wav ( -M model.wav [-A] | -C f0,f0[,f0...] ) [-L F0min (50)] [-H F0max (500)] "
                  "[-T hop_ms (10)] [-S seed] [flowgen_shimmer's -r -d -j -s -c -k -z -n -a -l]\n");
}

#define MAX_ANCHORS 256

int main(int argc, char **argv)
{
  const char *out = NULL, *model = NULL, *anchors = NULL, *seed_arg = NULL;
  int with_amp = 0;
  vs_pitch_opts po;
  vs_pitch_defaults(&po);
  /* flowgen_shimmer's own command line: its options as they stand, in their order */
  char **fg = (char **)calloc((size_t)argc + 4, sizeof(char *));
  int nfg = 0;
  if (!fg) return 1;
  fg[nfg++] = (char *)"vsource";
  fg[nfg++] = (char *)"-o";
  fg[nfg++] = (char *)"flow.wav";
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (strcmp(a, "-A") == 0) {
      with_amp = 1;
      continue;
    }
    if (a[0] != '-' || !a[1] || a[2] || !strchr("oMCLHTSrdjsckznal", a[1]) || i + 1 >= argc) goto bad_usage;
    const char *s = argv[++i];
    switch (a[1]) {
      case 'o': out = s; break;
      case 'M': model = s; break;
      case 'C': anchors = s; break;
      case 'S': seed_arg = s; break;
      case 'L': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; po.f0_min = (float)v; break;
      case 'H': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; po.f0_max = (float)v; break;
      case 'T': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; po.hop_s = v / 1000.0; break;
      default: fg[nfg++] = argv[i - 1]; fg[nfg++] = argv[i]; break;
    }
  }
  if (!out || (!model == !anchors) || (with_amp && !model)) goto bad_usage;
  vs_flowgen_cmd cmd;
  if (vs_flowgen_parse(nfg, fg, &cmd) != VS_OK) goto bad_usage;
  uint64_t seed = vs_cli_seed();
  if (seed_arg) {
    char *end = NULL;
    seed = (uint64_t)strtoull(seed_arg, &end, 0);
    if (!end || end == seed_arg || *end) goto bad_usage;
  }
  double f0s[MAX_ANCHORS];
  int n_anchors = 0;
  for (const char *s = anchors; s;) {
    char *end = NULL;
    const double v = strtod(s, &end);
    if (end == s || !isfinite(v) || !(v > 0.0) || n_anchors == MAX_ANCHORS) goto bad_usage;
    f0s[n_anchors++] = v;
    if (!*end) break;
    if (*end != ',') goto bad_usage;
    s = end + 1;
  }
  if (anchors && n_anchors < 2) goto bad_usage;
  free(fg);
  fg = NULL;

  VsWavRow mod, head;
  memset(&mod, 0, sizeof(mod));
  memset(&head, 0, sizeof(head));
  vs_pitch_frame *fr = NULL;
  int32_t *period = NULL, *amp = NULL;
  int16_t *flow = NULL;
  vs_ctx *ctx = NULL;
  int status = 1;
  vs_lane lane = cmd.lane;
  lane.seed = seed;
  vs_strack_row row;
  memset(&row, 0, sizeof(row));
  size_t N = 0;
  if (model) {
    if (vs_cli_read_wav("vsource", model, &mod) != 0) {
      status = 2;
      goto done;
    }
    lane.fs = mod.fs;
    N = (size_t)mod.len;
    if (vs_strack_from_pitch(&po, mod.fs, mod.len, &row) != VS_OK) {
      fprintf(stderr, "vsource: %s: no frame of the pitch track (%d samples at %d Hz, F0 %g..%g Hz, a hop of %g ms)\n", model,
              (int)mod.len, (int)mod.fs, (double)po.f0_min, (double)po.f0_max, po.hop_s * 1000.0);
      status = 2;
      goto done;
    }
    head = mod;
  } else {
    uint64_t ns = 0;
    const double lo = floor((double)lane.fs / (double)po.f0_max), hi = ceil((double)lane.fs / (double)po.f0_min);
    const double H = floor(po.hop_s * (double)lane.fs + 0.5);
    if (vs_num_samples(lane.fs, cmd.dur, &ns) != VS_OK || ns == 0 || ns > 0x7FFFFFFFu || !(lo >= 2.0) || !(lo <= hi) ||
        !(hi <= (double)VS_AC_MAX_LAG) || !(H >= 1.0) || !(H <= 2147483647.0))
      goto bad_usage;
    N = (size_t)ns;
    row.hop = (int32_t)H;
    row.n_frames = (int32_t)((N + (size_t)row.hop - 1) / (size_t)row.hop);
    row.offset = 0;
    row.length = (int32_t)N;
    row.pmin = (int32_t)lo;
    row.pmax = (int32_t)hi;
    head.hbytes = vs_wav_header_write(head.header, vs_cli_header_bytes(), lane.fs, cmd.dur);
    if (head.hbytes < 0) goto done;
  }
  const size_t F = (size_t)row.n_frames;
  period = (int32_t *)calloc(F, sizeof(int32_t));
  flow = (int16_t *)calloc(N ? N : 1, sizeof(int16_t));
  if (with_amp) amp = (int32_t *)calloc(F, sizeof(int32_t));
  if (model) fr = (vs_pitch_frame *)calloc(F, sizeof(vs_pitch_frame));
  if (!period || !flow || (with_amp && !amp) || (model && !fr)) {
    fprintf(stderr, "vsource: out of memory\n");
    goto done;
  }
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  int rc = VS_OK;
  if (model) {
    rc = vs_pitch(ctx, &po, mod.x, (size_t)mod.len, 1, (size_t)mod.len, &mod.fs, &mod.len, F, fr);
    if (rc != VS_OK) {
      fprintf(stderr, "vsource: %s\n", vs_strerror(rc));
      goto done;
    }
    int64_t rmax = 0;
    for (size_t f = 0; f < F; f++) {
      period[f] = fr[f].lag;
      if (fr[f].r0 > rmax) rmax = fr[f].r0;
    }
    for (size_t f = 0; with_amp && f < F; f++)
      amp[f] = rmax > 0 ? (int32_t)floor((double)lane.amp * sqrt((double)fr[f].r0 / (double)rmax) + 0.5) : 0;
  } else {
    for (size_t f = 0; f < F; f++) {
      size_t c = f * (size_t)row.hop + (size_t)(row.hop / 2);
      if (c > N) c = N;
      const double u = (double)c * (double)(n_anchors - 1) / (double)N;
      int k = (int)u;
      if (k > n_anchors - 2) k = n_anchors - 2;
      const double t = u - (double)k;
      const double f0 = f0s[k] + t * (f0s[k + 1] - f0s[k]);
      const double q = (double)lane.fs / f0;
      period[f] = (q >= 0.0 && q < 2147483647.0) ? (int32_t)q : 0;
    }
  }
  vs_strack_stat st;
  memset(&st, 0, sizeof(st));
  rc = vs_strack(ctx, NULL, &lane, 1, N, &row, period, F, amp, flow, &st, NULL, 0);
  if (rc != VS_OK) {
    fprintf(stderr, "vsource: %s\n", vs_strerror(rc));
    goto done;
  }
  int voiced = 0;
  for (size_t f = 0; f < F; f++)
    voiced += period[f] >= row.pmin && period[f] <= row.pmax && (!amp || (amp[f] >= 0 && amp[f] <= 32766));
  status = vs_cli_write_wav("vsource", out, &head, flow, N) == 0 ? 0 : 2;
  if (status == 0)
    printf("%s %d %d %d %d %d\n", out, (int)row.n_frames, voiced, (int)st.n_cycles, (int)st.n_resets, (int)st.status);
done:
  vs_ctx_destroy(ctx);
  free(fr);
  free(period);
  free(amp);
  free(flow);
  free(mod.x);
  return status;
bad_usage:
  free(fg);
  usage();
  return 1;
}
