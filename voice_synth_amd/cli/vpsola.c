/*
 * vpsola -- a recording with another F0, another cycle-to-cycle perturbation or another duration and its own waveform,
 * on the GPU: pitch-synchronous overlap-add of the file's own cycles (include/voice_synth.h, "PSOLA" and "PSOLA with a
 * time map").
 *
 *     vpsola -i in.wav -o out.wav [-x factor | -C f0,f0[,f0...]] [-j jitter_%] [-S seed] [-f F0min (50)] [-F F0max (500)]
 *            [-p polarity (1)] [-d factor] [-u unvoiced_ms (5)]
 *
 * One chain of launches on the device, over buffers that stay there: vs_pitch_launch (range -f..-F) -> vs_guided_launch
 * (VS_MG_ALL, polarity -p) -> [vs_strack_launch] -> vs_psola_launch with pmin and pmax the track's lag bounds.
 * The periods of the target, one per frame of the pitch track:
 *   neither -x nor -C: the track's own lags.
 *   -x factor: floor(lag / factor + 0.5) of every voiced frame (a lag inside the bounds); made on the HOST from the lags
 *       the pitch launch wrote, which come down for it.
 *   -C: two or more anchors in Hz spread evenly over the file, as vsource -C has them, on the frames of the pitch track:
 *       with c = min(f*H + C, N) the centre of frame f, F0_f is linear between the anchors at u = c * (n - 1) / N and the
 *       period is (int)(fs / F0_f) -- for the voiced frames only, also on the host.
 *   A period outside the bounds is a frame without a target: there the recording's own periods stand.
 * The target's cycles:
 *   -j: vs_strack_launch of a lane with that jitter (seed -S, else VS_SEED, else the clock) on the periods -- without -x
 *       and -C on the lag field of the pitch records, in place -- and its cycle log is the target, read in place (start
 *       and T at stride 32, n_cycles at stride 24): nothing comes down between the launches.
 *   without -j: the staircase of the periods, start and T by the source track's walk with T = P; that walk runs on the
 *       HOST and its two arrays go up.
 *   With none of -x, -C and -j the target has no cycle and the output is the input, byte for byte.
 * -d factor: the output is No = floor(N * factor + 0.5) samples long, through vs_psola_ts_launch with the map of the two
 *   anchors (0, 0) and (No, N) and the unvoiced period floor(unvoiced_ms * fs / 1000 + 0.5); the header's two sizes
 *   follow.  -d 1 is no change of duration: vs_psola_launch, the bytes and the line of a call without -d.  The target is
 *   in OUTPUT time, so with -x, -C or -j the period track is put there on the host (the lags come down for it): the
 *   output has the frames of vs_strack_from_pitch for No samples, and frame fo of them, which begins at
 *   g = min(offset + fo * hop, No - 1), has the period of the input's frame at the instant floor(g * N / No) -- the
 *   period -x or -C made of that frame, or its lag.  The staircase, or vs_strack_launch for -j, then runs over the No
 *   samples of the output on those periods.  With -d alone the target has no cycle: the duration changes, the pitch is
 *   the recording's.
 * stdout: one line "out.wav runs done synth governed clipped status" (the row's vs_psola_stat).
 * A file that cannot be read, has a truncated header, is not 16-bit PCM, has no samples, or whose rate and length give no
 * frame of the pitch track is named on stderr; the exit status is then 2.  Usage errors and device failures: 1.
 */
#include "cli_analysis.h"

static void usage(void)
{
  fprintf(stderr, "usage: vpsola -i in.wav -o out.wav [-x factor | -C f0,f0[,f0...]] [-j jitter_%%] [-S seed] [-f F0min (50)] "
                  "[-F F0max (500)] [-p polarity (1)] [-d factor] [-u unvoiced_ms (5)]\n");
}

#define MAX_ANCHORS 256

static int voiced(int32_t p, const vs_strack_row *row) { return p >= row->pmin && p <= row->pmax; }

/* the source track's walk (voice_synth.h, "source track", stages 1 and 2) with T = P: at most cap cycles */
static int32_t staircase(const int32_t *period, const vs_strack_row *row, int32_t *start, int32_t *T, int32_t cap)
{
  int32_t J = 0;
  int64_t g = 0;
  while (g < row->length && J < cap) {
    int64_t f = g < row->offset ? 0 : (g - row->offset) / row->hop;
    if (f > row->n_frames - 1) f = row->n_frames - 1;
    if (voiced(period[f], row)) {
      start[J] = (int32_t)g;
      T[J++] = period[f];
      g += period[f];
      continue;
    }
    int64_t f2 = f + 1;
    while (f2 < row->n_frames && !voiced(period[f2], row)) f2++;
    g = f2 < row->n_frames ? (int64_t)row->offset + f2 * row->hop : row->length;
  }
  return J;
}

/* the sizes of a header copied from the input, for n samples: the RIFF chunk's and the data chunk's, in either layout */
static void resize_header(VsWavRow *r, size_t n)
{
  const uint64_t data = (uint64_t)n * sizeof(int16_t), riff = data + 36;
  const int at_riff = r->hbytes == 72 ? 8 : 4, at_data = r->hbytes == 72 ? 64 : 40, width = r->hbytes == 72 ? 8 : 4;
  for (int k = 0; k < width; k++) {
    r->header[at_riff + k] = (unsigned char)(riff >> (8 * k));
    r->header[at_data + k] = (unsigned char)(data >> (8 * k));
  }
}

int main(int argc, char **argv)
{
  const char *in = NULL, *out = NULL, *anchors = NULL, *seed_arg = NULL, *jitter_arg = NULL;
  double factor = 0.0, stretch = 0.0, unvoiced_ms = 5.0;
  vs_guided_opts go;
  vs_guided_defaults(&go);
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    double v = 0.0;
    if (a[0] != '-' || !a[1] || a[2] || !strchr("ioxCjSfFpdu", a[1]) || i + 1 >= argc) goto bad_usage;
    const char *s = argv[++i];
    switch (a[1]) {
      case 'i': in = s; break;
      case 'o': out = s; break;
      case 'C': anchors = s; break;
      case 'S': seed_arg = s; break;
      case 'j': if (!number(s, &v) || !(v >= 0.0)) goto bad_usage; jitter_arg = s; break;
      case 'x': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; factor = v; break;
      case 'd': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; stretch = v; break;
      case 'u': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; unvoiced_ms = v; break;
      case 'f': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; go.f0_min = (float)v; break;
      case 'F': if (!number(s, &v) || !(v > 0.0)) goto bad_usage; go.f0_max = (float)v; break;
      default: if (!number(s, &v) || (v != 1.0 && v != -1.0)) goto bad_usage; go.polarity = (int32_t)v; break;
    }
  }
  if (!in || !out || (factor != 0.0 && anchors)) goto bad_usage;
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
  vs_lane lane;
  memset(&lane, 0, sizeof(lane));
  if (jitter_arg) { /* the lane of "flowgen_shimmer -j jitter" */
    char *fg[5] = {(char *)"vpsola", (char *)"-o", (char *)"flow.wav", (char *)"-j", (char *)jitter_arg};
    vs_flowgen_cmd cmd;
    if (vs_flowgen_parse(5, fg, &cmd) != VS_OK) goto bad_usage;
    lane = cmd.lane;
    lane.seed = seed;
  }

  VsWavRow src;
  memset(&src, 0, sizeof(src));
  int status = 1;
  vs_ctx *ctx = NULL;
  void *d_pcm = NULL, *d_fr = NULL, *d_meas = NULL, *d_marks = NULL, *d_rec = NULL, *d_segs = NULL, *d_tgt = NULL,
       *d_count = NULL, *d_flow = NULL, *d_cyc = NULL, *d_sst = NULL, *d_out = NULL, *d_stat = NULL, *d_synth = NULL,
       *d_map = NULL;
  vs_pitch_frame *fr = NULL;
  int32_t *tgt = NULL;
  int16_t *y = NULL;
  if (vs_cli_read_wav("vpsola", in, &src) != 0) return 2;
  if (src.len == 0) {
    fprintf(stderr, "vpsola: %s: no samples\n", in);
    status = 2;
    goto done;
  }
  vs_pitch_opts po;
  vs_pitch_defaults(&po);
  po.f0_min = go.f0_min;
  po.f0_max = go.f0_max;
  po.hop_s = go.hop_s;
  vs_strack_row row;
  int32_t tmin = 0, tmax = 0, H = 0, F = 0, centre = 0;
  if (vs_strack_from_pitch(&po, src.fs, src.len, &row) != VS_OK ||
      vs_guided_plan(&go, src.fs, src.len, &tmin, &tmax, &H, &F, &centre) != VS_OK || F < 1) {
    fprintf(stderr, "vpsola: %s: no frame of the pitch track (%d samples at %d Hz, F0 %g..%g Hz)\n", in, (int)src.len,
            (int)src.fs, (double)go.f0_min, (double)go.f0_max);
    status = 2;
    goto done;
  }
  lane.fs = src.fs;
  const size_t N = (size_t)src.len, nF = (size_t)F;
  /* the output: No samples; with a change of duration its own frames, on which the target's periods lie */
  const int ts = stretch != 0.0 && stretch != 1.0;
  const double want = ts ? floor((double)N * stretch + 0.5) : (double)N;
  vs_strack_row orow = row;
  const double uq = floor(unvoiced_ms * (double)src.fs / 1000.0 + 0.5);
  const int32_t U = uq < 2147483647.0 ? (int32_t)uq : 0; /* (out of range: the launch says so) */
  if (!(want >= 1.0 && want <= 2147483647.0) || (ts && vs_strack_from_pitch(&po, src.fs, (int32_t)want, &orow) != VS_OK)) {
    fprintf(stderr, "vpsola: %s: no frame of the pitch track in an output of %.0f samples\n", in, want);
    status = 2;
    goto done;
  }
  const size_t No = (size_t)want, nFo = ts ? (size_t)orow.n_frames : nF;
  const int32_t len_out = (int32_t)No;
  const size_t least = ts && (size_t)(U / 2 + 1) < (size_t)tmin ? (size_t)(U / 2 + 1) : (size_t)tmin;
  const size_t mp = N / (size_t)tmin + 2, sp = nF, cap = (No > N ? No : N) / (size_t)tmin + 2;
  const size_t yp = ts ? No / (least ? least : 1) + 2 * sp + 4 : mp + 2 * sp + 2;
  const int own_periods = factor != 0.0 || anchors != NULL; /* the periods are made here, not the track's lags */
  const int host_periods = own_periods || (ts && jitter_arg); /* ... or put into output time here */
  fr = (vs_pitch_frame *)calloc(nF, sizeof(vs_pitch_frame));
  tgt = (int32_t *)calloc(2 * cap + nF + nFo, sizeof(int32_t)); /* start [cap], T [cap]; the periods [F]; the output's [Fo] */
  y = (int16_t *)calloc(No, sizeof(int16_t));
  if (!fr || !tgt || !y) {
    fprintf(stderr, "vpsola: out of memory\n");
    goto done;
  }
  int32_t *start = tgt, *T = tgt + cap, *period = tgt + 2 * cap, *operiod = ts ? period + nF : period;
  if (vs_cli_open_ctx(&ctx) != VS_OK) goto done;
  int rc = VS_OK;
#define TRY(call)                                           \
  do {                                                      \
    rc = (call);                                            \
    if (rc != VS_OK) {                                      \
      fprintf(stderr, "vpsola: %s\n", vs_strerror(rc));     \
      goto done;                                            \
    }                                                       \
  } while (0)
  TRY(vs_dev_alloc(ctx, N * sizeof(int16_t), &d_pcm));
  TRY(vs_dev_alloc(ctx, nF * sizeof(vs_pitch_frame), &d_fr));
  TRY(vs_dev_alloc(ctx, sizeof(vs_acoustic), &d_meas));
  TRY(vs_dev_alloc(ctx, mp * sizeof(int32_t), &d_marks));
  TRY(vs_dev_alloc(ctx, sizeof(vs_guided_rec), &d_rec));
  TRY(vs_dev_alloc(ctx, sp * sizeof(vs_guided_seg), &d_segs));
  TRY(vs_dev_alloc(ctx, (2 * cap + nF + nFo) * sizeof(int32_t), &d_tgt));
  TRY(vs_dev_alloc(ctx, sizeof(int32_t), &d_count));
  TRY(vs_dev_alloc(ctx, No * sizeof(int16_t), &d_out));
  TRY(vs_dev_alloc(ctx, sizeof(vs_psola_stat), &d_stat));
  TRY(vs_dev_alloc(ctx, yp * sizeof(vs_psola_mark), &d_synth));
  TRY(vs_dev_upload(ctx, d_pcm, src.x, N * sizeof(int16_t)));
  TRY(vs_dev_upload(ctx, d_fr, fr, nF * sizeof(vs_pitch_frame)));
  TRY(vs_pitch_launch(ctx, &po, (const int16_t *)d_pcm, N, 1, N, &src.fs, &src.len, nF, (vs_pitch_frame *)d_fr));
  TRY(vs_guided_launch(ctx, &go, (const int16_t *)d_pcm, N, 1, N, &src.fs, &src.len, (const vs_pitch_frame *)d_fr, nF,
                       (vs_acoustic *)d_meas, (int32_t *)d_marks, mp, (vs_guided_rec *)d_rec, (vs_guided_seg *)d_segs,
                       sp));
  int32_t J = 0;
  if (host_periods) {
    TRY(vs_dev_download(ctx, fr, d_fr, nF * sizeof(vs_pitch_frame)));
    for (size_t f = 0; f < nF; f++) {
      const int32_t lag = fr[f].lag;
      period[f] = 0;
      if (!voiced(lag, &row)) continue;
      double q;
      if (anchors) {
        size_t c = f * (size_t)H + (size_t)centre;
        if (c > N) c = N;
        const double u = (double)c * (double)(n_anchors - 1) / (double)N;
        int k = (int)u;
        if (k > n_anchors - 2) k = n_anchors - 2;
        q = (double)src.fs / (f0s[k] + (u - (double)k) * (f0s[k + 1] - f0s[k]));
      } else if (factor != 0.0) {
        q = floor((double)lag / factor + 0.5);
      } else {
        q = (double)lag;
      }
      period[f] = (q >= 0.0 && q < 2147483647.0) ? (int32_t)q : 0;
    }
    if (ts) /* into output time: the period of the input's frame at the instant the map gives the output frame's first */
      for (size_t fo = 0; fo < nFo; fo++) {
        int64_t g = (int64_t)orow.offset + (int64_t)fo * orow.hop;
        if (g > (int64_t)No - 1) g = (int64_t)No - 1;
        const int64_t at = g * (int64_t)N / (int64_t)No;
        int64_t f = at < row.offset ? 0 : (at - row.offset) / row.hop;
        if (f > (int64_t)nF - 1) f = (int64_t)nF - 1;
        operiod[fo] = period[f];
      }
    if (!jitter_arg) J = staircase(operiod, &orow, start, T, (int32_t)cap);
    TRY(vs_dev_upload(ctx, d_tgt, tgt, (2 * cap + nF + nFo) * sizeof(int32_t)));
  }
  const int32_t *start_dev = (const int32_t *)d_tgt, *period_dev = (const int32_t *)d_tgt + cap;
  const int32_t *count_dev = (const int32_t *)d_count;
  size_t tstride = sizeof(int32_t), cstride = sizeof(int32_t);
  if (jitter_arg) {
    TRY(vs_dev_alloc(ctx, No * sizeof(int16_t), &d_flow));
    TRY(vs_dev_alloc(ctx, cap * sizeof(vs_strack_cycle), &d_cyc));
    TRY(vs_dev_alloc(ctx, sizeof(vs_strack_stat), &d_sst));
    const int32_t *per = host_periods ? (const int32_t *)d_tgt + (operiod - tgt) : &((const vs_pitch_frame *)d_fr)->lag;
    TRY(vs_strack_launch(ctx, NULL, &lane, 1, No, &orow, per, host_periods ? sizeof(int32_t) : sizeof(vs_pitch_frame), nFo,
                         NULL, 0, (int16_t *)d_flow, No, (vs_strack_stat *)d_sst, (vs_strack_cycle *)d_cyc, cap));
    start_dev = &((const vs_strack_cycle *)d_cyc)->start;
    period_dev = &((const vs_strack_cycle *)d_cyc)->T;
    count_dev = &((const vs_strack_stat *)d_sst)->n_cycles;
    tstride = sizeof(vs_strack_cycle);
    cstride = sizeof(vs_strack_stat);
  } else {
    TRY(vs_dev_upload(ctx, d_count, &J, sizeof(J)));
  }
  if (ts) {
    struct {
      vs_psola_anchor an[2];
      int32_t w;
    } map = {{{0, 0}, {len_out, src.len}}, 2};
    vs_psola_ts_opts pto;
    vs_psola_ts_defaults(&pto);
    pto.pmin = tmin;
    pto.pmax = tmax;
    pto.unvoiced_period = U;
    TRY(vs_dev_alloc(ctx, sizeof(map), &d_map));
    TRY(vs_dev_upload(ctx, d_map, &map, sizeof(map)));
    TRY(vs_psola_ts_launch(ctx, &pto, (const int16_t *)d_pcm, N, 1, N, &src.len, (const int32_t *)d_marks, mp,
                           (const vs_guided_rec *)d_rec, (const vs_guided_seg *)d_segs, sp, start_dev, tstride, period_dev,
                           tstride, NULL, 0, count_dev, cstride, cap, (const vs_psola_anchor *)d_map,
                           (const int32_t *)((const char *)d_map + sizeof(map.an)), 2, (int16_t *)d_out, No, No, &len_out,
                           (vs_psola_stat *)d_stat, (vs_psola_mark *)d_synth, yp));
    resize_header(&src, No);
  } else {
    vs_psola_opts pso;
    vs_psola_defaults(&pso);
    pso.pmin = tmin;
    pso.pmax = tmax;
    TRY(vs_psola_launch(ctx, &pso, (const int16_t *)d_pcm, N, 1, N, &src.len, (const int32_t *)d_marks, mp,
                        (const vs_guided_rec *)d_rec, (const vs_guided_seg *)d_segs, sp, start_dev, tstride, period_dev,
                        tstride, NULL, 0, count_dev, cstride, cap, (int16_t *)d_out, N, (vs_psola_stat *)d_stat,
                        (vs_psola_mark *)d_synth, yp));
  }
  vs_psola_stat st;
  TRY(vs_dev_download(ctx, y, d_out, No * sizeof(int16_t)));
  TRY(vs_dev_download(ctx, &st, d_stat, sizeof(st)));
  status = vs_cli_write_wav("vpsola", out, &src, y, No) == 0 ? 0 : 2;
  if (status == 0)
    printf("%s %d %d %d %d %d %d\n", out, (int)st.n_runs, (int)st.n_runs_done, (int)st.n_synth, (int)st.n_governed,
           (int)st.n_clipped, (int)st.status);
done:
  if (ctx) {
    void *bufs[] = {d_pcm, d_fr, d_meas, d_marks, d_rec, d_segs, d_tgt, d_count, d_flow, d_cyc, d_sst, d_out, d_stat, d_synth, d_map};
    for (size_t k = 0; k < sizeof(bufs) / sizeof(bufs[0]); k++)
      if (bufs[k]) vs_dev_free(ctx, bufs[k]);
  }
  vs_ctx_destroy(ctx);
  free(fr);
  free(tgt);
  free(y);
  free(src.x);
  return status;
bad_usage:
  usage();
  return 1;
}
